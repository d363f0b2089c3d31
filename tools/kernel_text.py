"""Per-kernel comparison of the gfx950 device assembly of two builds: has a source change altered the generated code?

    hipcc <the Makefile's CXXFLAGS> --cuda-device-only -S x.hip -o x.s      (for every unit, before and after)
    python tools/kernel_text.py --before old/wb_channels.s --after new/wb_channels.s new/wb_chan_u1.s ...

A kernel's text is what stands between its label and .Lfunc_end, without comments and without the directives and label
numbers that only follow its position in the file.  Prints one line per kernel -- `same`, or the instruction counts and the
descriptor values (VGPRs, SGPRs, LDS bytes, scratch bytes) of both sides -- and exits 1 if any kernel differs or is missing."""
import argparse
import re
import sys

DIRECTIVES = re.compile(r"^\.(file|loc|ident|p2align|type|size|globl|protected|section|text|weak|hidden)\b")
DESCRIPTOR = ("next_free_vgpr", "next_free_sgpr", "group_segment_fixed_size", "private_segment_fixed_size")


def kernels(paths):
    """{kernel name: (body lines, descriptor values)} of the .amdhsa_kernel entries of the given .s files."""
    out = {}
    for path in paths:
        text = open(path).read()
        for name, desc in re.findall(r"^\s*\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", text, re.M | re.S):
            body = re.search(r"^" + re.escape(name) + r":[^\n]*\n(.*?)^\.Lfunc_end", text, re.M | re.S).group(1)
            lines = [re.sub(r"\.LBB\d+_", ".LBB_", ln.split(";")[0].strip()) for ln in body.split("\n")]
            lines = [ln for ln in lines if ln and not DIRECTIVES.match(ln)]
            out[name] = (lines, tuple(int(re.search(r"\.amdhsa_%s (\d+)" % k, desc).group(1)) for k in DESCRIPTOR))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--before", nargs="+", required=True)
    ap.add_argument("--after", nargs="+", required=True)
    args = ap.parse_args()
    old, new = kernels(args.before), kernels(args.after)
    n_insts = lambda lines: sum(1 for ln in lines if not ln.endswith(":"))
    same = 0
    for name in sorted(set(old) | set(new)):
        if name not in old or name not in new:
            print(f"{name}: only {'before' if name in old else 'after'}")
        elif old[name] == new[name]:
            print(f"{name}: same ({n_insts(new[name][0])} instructions)")
            same += 1
        else:
            print(f"{name}: DIFFERS  instructions {n_insts(old[name][0])} -> {n_insts(new[name][0])}  "
                  f"(vgpr, sgpr, lds, scratch) {old[name][1]} -> {new[name][1]}")
    differ = len(set(old) | set(new)) - same
    print(f"{len(new)} kernels, {same} identical, {differ} differ or are missing")
    sys.exit(1 if differ else 0)


if __name__ == "__main__":
    main()
