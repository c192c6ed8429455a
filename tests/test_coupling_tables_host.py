"""The coupling-table test of the chunk sweep and its back-substitution (csrc/bcr_dev.hpp: right_table_is_interior), on the
host through acino_debug_coupling_table: where it says "interior" the evaluated band IS the constant table {-1, 6, -15}, and it
says so for every node that lies inside its sequence or clip - the test is exact, not conservative."""
import ctypes as C

import pytest

from acinoset_amd import _lib

INTERIOR = (-1.0, 6.0, -15.0, 0.0, -1.0, 6.0, 0.0, 0.0, -1.0)      # [3 ii + jj]: {-1, 6, -15}[jj - ii], ii <= jj


@pytest.fixture(scope="module")
def table():
    fn = _lib.lib().acino_debug_coupling_table
    flag, coef = C.c_int32(), (C.c_double * 9)()

    def call(n_global, n_frames, n_offset, clip_len, pin_left, node):
        assert fn(n_global, n_frames, n_offset, clip_len, pin_left, node, C.byref(flag), coef) == 0
        return bool(flag.value), tuple(coef)
    return call


def windows(n_global):
    """(n_offset, n_frames): the whole sequence, and windows that start and end at every residue of a node and of a clip."""
    yield 0, n_global
    for off in (1, 2, 3, 5, 6, 7, 12, 13):
        for nf in (1, 2, 3, 4, 6, 7, 11, 12, n_global - off - 2, n_global - off - 1, n_global - off):
            if off < n_global and 1 <= nf and off + nf <= n_global:
                yield off, nf


def six_frames_inside(n_global, n_frames, n_offset, clip_len, pin_left, node):
    """The six frames the table couples (the node's three and its right neighbour's) are frames of the window and lie at
    least six frames inside the sequence, or inside one clip (complete or cut by the end of the sequence)."""
    loc = 3 * (node - pin_left)
    f = n_offset + loc
    if f < 0 or loc + 5 >= n_frames:
        return False
    if clip_len == 0:
        return f >= 6 and f + 5 <= n_global - 1 - 6
    lo = f // clip_len * clip_len
    return f - lo >= 6 and f + 5 <= min(lo + clip_len, n_global) - 1 - 6 and lo + clip_len <= n_global


@pytest.mark.parametrize("clip_len", [0, 6, 7, 12])
@pytest.mark.parametrize("pin_left", [0, 1])
def test_interior_means_the_constant_table_and_inside_means_interior(table, clip_len, pin_left):
    n_true = n_inside = 0
    for n_global in range(1, 65):
        for n_offset, n_frames in windows(n_global):
            n_nodes = pin_left + (n_frames + 2) // 3
            for node in range(pin_left - 1, n_nodes + 1):           # (pin_left - 1: the left table of the first node)
                args = (n_global, n_frames, n_offset, clip_len, pin_left, node)
                interior, coef = table(*args)
                if interior:
                    n_true += 1
                    assert coef == INTERIOR, args
                else:
                    assert coef != INTERIOR, args                   # exact: never the constants where the test says no
                if six_frames_inside(*args):
                    n_inside += 1
                    assert interior, args
    assert n_true > 0
    assert n_inside > 0 or clip_len > 0                             # (a clip of <= 12 frames has no node six frames inside)


def test_the_last_interior_node_of_a_long_run_is_interior(table):
    # 10 000 frames, no pin: the last full-length run of the benchmark ends with the node of frames 9990 .. 9992, whose right
    # table reaches frame 9995 <= 9999 - the run a test "conservative by a node" sent through the evaluation on every node
    assert table(10000, 10000, 0, 0, 0, 3330) == (True, INTERIOR)
    assert table(10000, 10000, 0, 0, 0, 3331) == (True, INTERIOR)   # frames 9993 .. 9998: the last complete third-difference rows
    assert table(10000, 10000, 0, 0, 0, 3332)[0] is False         # frames 9996 .. 10001: beyond the sequence
    assert table(10000, 10000, 0, 0, 0, 0) == (True, INTERIOR)    # frames 0 .. 5: band_coef's interior branch from row 3 - 3
    assert table(10000, 10000, 0, 0, 0, -1)[0] is False           # the left table of node 0: nothing on its left
