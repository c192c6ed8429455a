#!/usr/bin/env python3
"""Compare the gfx950 device code of HIP sources in two trees of this project, kernel by kernel.

    python scripts/isa_diff.py PARENT_TREE THIS_TREE file.hip ... [--rename 'old=new' ...]

Every file is compiled in both trees with build()'s flags (acinoset_amd/_lib.py: HIPCC_FLAGS) plus
``--cuda-device-only -S``, at most 16 compilations at a time.  The assembly is cut into functions - from a function's
label to its ``.Lfunc_end``, plus the ``.amdhsa_kernel`` descriptor of a kernel - and what differs between two
compilations of the same code is masked: the function's own symbol, ``__hip_cuid_*``, the function counter in local labels
(``.LBB<k>_<n>``, ``.Lfunc_end<k>``), section directives and assembler comments.  Per file it prints the difference of the symbol sets, which
functions are identical and, for the rest, the first differing lines and the descriptor fields that differ.

A function that exists under the same symbol in both trees is compared with itself.  ``--rename`` pairs two that do not: both
sides are demangled names without the return type, the namespace and the parameter list, e.g.
``--rename 'k_fte_assemble_pinhole<true, 1>=k_fte_assemble<true, 0, 1, true>'``.  What is left is paired by body: a function
of the parent whose masked text equals that of a new function of this tree is that function under a new name.

A text comparison of two compilations; it looks for nothing in particular.  Exit status 0: same symbols up to the renames,
every function identical; 1 otherwise.
"""
import argparse
import importlib.util
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

LINES_SHOWN = 6


def hipcc_flags(tree):
    spec = importlib.util.spec_from_file_location("_isa_diff_lib", os.path.join(tree, "acinoset_amd", "_lib.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return list(mod.HIPCC_FLAGS)


def compile_asm(hipcc, flags, tree, name, out):
    cmd = [hipcc] + flags + ["--cuda-device-only", "-S", os.path.join(tree, "acinoset_amd", "csrc", name), "-o", out]
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError(f"hipcc failed on {name} in {tree}:\n" + res.stderr[-4000:])
    with open(out) as f:
        return f.read()


_MASKS = [(re.compile(r"__hip_cuid_[0-9a-f]+"), "__hip_cuid"),
          (re.compile(r"\.L(BB|JTI|func_begin|func_end|tmp)(\d+)(_\d+)?"), lambda m: f".L{m.group(1)}{m.group(3) or ''}")]


def _mask(line, sym):
    line = line.split(";", 1)[0].rstrip()                  # assembler comments
    if line.strip() == ".text" or line.lstrip().startswith(".section"):
        return ""                                          # (a plain function ends in .text, a template instantiation in a comdat section)
    line = line.replace(sym, "<self>")
    for pat, rep in _MASKS:
        line = pat.sub(rep, line)
    return line


def split_functions(asm):
    """{symbol: (code lines, descriptor lines)}, masked; the descriptor is empty for a function that is no kernel."""
    lines = asm.splitlines()
    syms = [m.group(1) for m in (re.match(r"\s*\.type\s+(\S+),@function", ln) for ln in lines) if m]
    out = {}
    for sym in syms:
        lo = next((i for i, ln in enumerate(lines) if ln.split(";", 1)[0].rstrip() == sym + ":"), None)
        if lo is None:
            continue
        hi = next(i for i in range(lo, len(lines)) if re.match(r"\.Lfunc_end\d+:", lines[i]))
        code = [x for x in (_mask(ln, sym) for ln in lines[lo:hi + 1]) if x.strip()]
        desc = []
        head = "\t.amdhsa_kernel " + sym
        if head in lines:
            d0 = lines.index(head)
            d1 = next(i for i in range(d0, len(lines)) if lines[i].strip() == ".end_amdhsa_kernel")
            desc = [x for x in (_mask(ln, sym) for ln in lines[d0:d1 + 1]) if x.strip()]
        out[sym] = (code, desc)
    return out


def demangle(cxxfilt, syms):
    if not syms:
        return {}
    res = subprocess.run([cxxfilt], input="\n".join(syms) + "\n", capture_output=True, text=True)
    names = res.stdout.splitlines() if res.returncode == 0 else syms
    return dict(zip(syms, names))


def short(name):
    """'void acino::k<true, 1>(args)' -> 'k<true, 1>'"""
    depth, cut = 0, len(name)
    for i, ch in enumerate(name):
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        elif ch == "(" and depth == 0:
            cut = i
            break
    head = name[:cut]
    head = head.split(" ", 1)[1] if head.startswith("void ") else head
    return head.replace("acino::", "")


def describe(a, b):
    (ca, da), (cb, db) = a, b
    msgs = []
    if ca != cb:
        i = next((k for k, (x, y) in enumerate(zip(ca, cb)) if x != y), min(len(ca), len(cb)))
        msgs.append(f"      code: {len(ca)} / {len(cb)} lines, first difference at line {i + 1}")
        for k in range(i, min(i + LINES_SHOWN, max(len(ca), len(cb)))):
            msgs.append(f"        - {ca[k].strip() if k < len(ca) else '<end>'}")
            msgs.append(f"        + {cb[k].strip() if k < len(cb) else '<end>'}")
    if da != db:
        fa = dict(ln.split(None, 1) if " " in ln.strip() else (ln, "") for ln in (x.strip() for x in da))
        fb = dict(ln.split(None, 1) if " " in ln.strip() else (ln, "") for ln in (x.strip() for x in db))
        for key in sorted(set(fa) | set(fb)):
            if fa.get(key) != fb.get(key):
                msgs.append(f"      descriptor {key}: {fa.get(key)} -> {fb.get(key)}")
    return msgs


def compare(name, old, new, renames, cxxfilt):
    names = demangle(cxxfilt, sorted(set(old) | set(new)))
    label = {s: short(names[s]) for s in names}
    pairs = [(s, s) for s in old if s in new]
    lost = [s for s in old if s not in new]
    born = [s for s in new if s not in old]
    how = {}
    for a, b in renames:
        sa = [s for s in lost if label[s] == a]
        sb = [s for s in born if label[s] == b]
        if len(sa) == 1 and len(sb) == 1:
            pairs.append((sa[0], sb[0]))
            how[sa[0]] = "--rename"
            lost.remove(sa[0])
            born.remove(sb[0])
    for s in list(lost):                                   # what is left: the same body under a new name
        same = [t for t in born if new[t] == old[s]]       # (several when two instantiations compile to the same code:
        if same:                                           #  the one whose name shares the longest prefix)
            t = max(same, key=lambda t: len(os.path.commonprefix([label[s].rstrip(">"), label[t]])))
            pairs.append((s, t))
            how[s] = "matched by body"
            lost.remove(s)
            born.remove(t)
    guess = {}                                             # neither: show the nearest name's difference, still counted as lost + new
    for s in lost:
        if born:
            guess[s] = max(born, key=lambda t: len(os.path.commonprefix([label[s].rstrip(">"), label[t]])))
    print(f"== {name}: {len(old)} functions in the parent, {len(new)} in this tree")
    print(f"   symbols: {len(lost)} only in the parent, {len(born)} only in this tree, "
          f"{sum(1 for a, b in pairs if a != b)} renamed")
    for s in lost:
        print(f"   ONLY IN THE PARENT  {label[s]}")
        if s in guess:
            print(f"      against {label[guess[s]]}:")
            for m in describe(old[s], new[guess[s]]):
                print(m)
    for s in born:
        print(f"   ONLY IN THIS TREE   {label[s]}")
    bad = len(lost) + len(born)
    for a, b in sorted(pairs, key=lambda p: label[p[1]]):
        kind = "kernel" if old[a][1] else "function"
        tag = f"{label[b]}" if a == b else f"{label[a]}  ->  {label[b]}  ({how[a]})"
        if old[a] == new[b]:
            print(f"   identical  {kind}  {tag}   [{len(old[a][0])} lines]")
        else:
            bad += 1
            print(f"   DIFFERENT  {kind}  {tag}")
            for m in describe(old[a], new[b]):
                print(m)
    return bad


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("parent_tree")
    ap.add_argument("this_tree")
    ap.add_argument("files", nargs="+", help="names under acinoset_amd/csrc, e.g. ekf.hip")
    ap.add_argument("--rename", action="append", default=[], metavar="OLD=NEW")
    ap.add_argument("--jobs", type=int, default=16)
    args = ap.parse_args()
    renames = [tuple(x.strip() for x in r.split("=", 1)) for r in args.rename]
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    hipcc = os.environ.get("HIPCC", os.path.join(rocm, "bin", "hipcc"))
    cxxfilt = os.path.join(rocm, "llvm", "bin", "llvm-cxxfilt")
    if not os.path.exists(cxxfilt):
        cxxfilt = "c++filt"
    flags = hipcc_flags(args.this_tree)
    print("flags: " + " ".join(flags) + " --cuda-device-only -S")
    with tempfile.TemporaryDirectory() as tmp:
        jobs = [(tree, f, os.path.join(tmp, f"{side}_{f}.s"))
                for f in args.files for side, tree in (("parent", args.parent_tree), ("this", args.this_tree))]
        with ThreadPoolExecutor(max_workers=max(1, min(16, args.jobs))) as ex:
            asm = list(ex.map(lambda j: compile_asm(hipcc, flags, *j), jobs))
    bad = 0
    for i, f in enumerate(args.files):
        bad += compare(f, split_functions(asm[2 * i]), split_functions(asm[2 * i + 1]), renames, cxxfilt)
    print(f"== {'every function identical, symbol sets equal up to the renames' if bad == 0 else f'{bad} differences'}")
    return 0 if bad == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
