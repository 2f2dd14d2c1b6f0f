#!/usr/bin/env python3
"""Compare the gfx950 code of every kernel of two checkouts, as text.  CPU only: it compiles, it runs nothing.

  python tools/kernel_isa_diff.py <parent checkout> <this tree> [--allow KERNEL ...]

Every ecckd_amd/csrc/*.hip of each checkout is compiled with the Makefile's HIPFLAGS, `-shared` replaced by
`--cuda-device-only -cuid=fixed -S`, and each .s is cut at its kernel symbols.  Per kernel it prints `identical`, or both
sides' instruction counts and `.vgpr_count / .sgpr_count / .private_segment_fixed_size / .group_segment_fixed_size`.
The exit status is 1 if a kernel differs whose name is not in --allow (kernels of --allow are printed with their counts
either way).  Instruction text means: labels and instructions without comments, basic-block labels without the number of
the function in its file."""
import argparse, concurrent.futures, pathlib, re, subprocess, sys, tempfile

FIELDS = ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")


def hipflags(tree):
    mk = (tree / "Makefile").read_text()
    flags = re.search(r"^HIPFLAGS \?= (.*)$", mk, re.M).group(1).split()
    hipcc = re.search(r"^HIPCC \?= (.*)$", mk, re.M).group(1).strip()
    return hipcc, [f for f in flags if f != "-shared"] + ["--cuda-device-only", "-cuid=fixed", "-S"]


def kernels(tree, src, out):
    """{symbol: (instruction lines, counts)} of one .hip file"""
    hipcc, flags = hipflags(tree)
    subprocess.run([hipcc, *flags, "-o", str(out), str(src)], check=True, cwd=tree, stderr=subprocess.DEVNULL)
    text = out.read_text()
    meta = {}
    for entry in text[text.find(".amdgpu_metadata"):].split("\n  - ")[1:]:
        sym = re.search(r"^    \.symbol:\s+(\S+)\.kd$", entry, re.M)
        if not sym: continue   # a list of the metadata that is not the kernels'
        sym = sym.group(1)
        meta[sym] = " / ".join(re.search(rf"^    \.{f}:\s+(\d+)$", entry, re.M).group(1) for f in FIELDS)
    found = {}
    for sym in meta:
        body = text[text.index(f"\n{sym}:"):]
        body = body[:body.index("\n.Lfunc_end")]
        lines = (re.sub(r"\.LBB\d+_", ".LBB_", ln.split(";")[0].strip()) for ln in body.splitlines())
        found[sym] = ([ln for ln in lines if ln and (not ln.startswith(".") or ln.endswith(":"))], meta[sym])
    return found


def ninstr(lines):
    return sum(not ln.endswith(":") for ln in lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("parent", type=pathlib.Path)
    ap.add_argument("branch", type=pathlib.Path)
    ap.add_argument("--allow", nargs="*", default=[], help="kernel names (unmangled, without template arguments) that may differ")
    ap.add_argument("-j", type=int, default=8)
    args = ap.parse_args()
    names = sorted({p.name for t in (args.parent, args.branch) for p in (t / "ecckd_amd/csrc").glob("*.hip")})
    bad = 0
    with tempfile.TemporaryDirectory() as tmp, concurrent.futures.ThreadPoolExecutor(args.j) as pool:
        def side(tree, tag, name):
            src = tree.resolve() / "ecckd_amd/csrc" / name
            return pool.submit(kernels, tree.resolve(), src, pathlib.Path(tmp) / f"{tag}_{name}.s") if src.exists() else None
        jobs = [(n, side(args.parent, "a", n), side(args.branch, "b", n)) for n in names]
        for name, ja, jb in jobs:
            a, b = (j.result() if j else {} for j in (ja, jb))
            print(f"## {name}: {len(b)} kernels")
            for sym in sorted(set(a) | set(b)):
                allowed = any(sym == k or f"{len(k)}{k}" in sym for k in args.allow)
                (ia, ma), (ib, mb) = a.get(sym, ([], "absent")), b.get(sym, ([], "absent"))
                same = sym in a and sym in b and ia == ib and ma == mb
                if same and not allowed:
                    print(f"{sym}: identical")
                else:
                    print(f"{sym}: {'identical' if same else 'DIFFERS'}{' (allowed)' if allowed else ''}: "
                          f"parent {ninstr(ia)} instructions, {ma}; branch {ninstr(ib)} instructions, {mb}")
                    bad += not same and not allowed
    print(f"{bad} kernel(s) differ outside --allow")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
