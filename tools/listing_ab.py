"""Compare two gfx950 listings of the library (csrc/build/ncsnpp-hip-amdgcn-amd-amdhsa-gfx950.s of two builds, e.g. the parent commit's and this one's), kernel by kernel:
which kernel symbols each has, and for the kernels whose names match ``--match`` (default: the stream-writing instances the stream guard has twins of) the opcode
counts and the register allocation side by side.  Host code only:

    python tools/listing_ab.py PARENT.s THIS.s [--also THIS_OTHER_UNIT.s] [--match REGEX] > profiles/stream_guard/listing_ab.txt

``--also``: a second listing of this build whose kernels are added to THIS's (a translation unit the parent does not have, e.g. stream_guard); kernels it holds under
the name of one THIS holds already -- the shared headers' non-template kernels, compiled into every unit that includes them -- are left out.
"""
import argparse
import re
import subprocess
from collections import Counter

STREAM_WRITERS = (r"k_gemm_(dma|ring)I.*Li(7|10)EEEv|k_gemm_w128ILi(7|10)E|k_gemm_(w128_)?fp8ILb[01]ELi[34]EE|k_splitk_reduce_f32|k_patch_embed")


def parse(path):
    text = open(path).read()
    bodies = {m.group(1): m.group(2) for m in re.finditer(r"^(_Z\w+):\s*(?:;[^\n]*)?\n(.*?)^\.Lfunc_end\d+:", text, re.M | re.S)}
    out = {}
    md = text[text.index("amdhsa.kernels:"):]
    for blk in re.split(r"\n  - \.", md)[1:]:
        name = re.search(r"\.name:\s*(\S+)", blk).group(1)

        def get(key):
            m = re.search(r"\." + key + r":\s*(\S+)", blk)
            return int(m.group(1)) if m else 0
        ops = Counter(m.group(1) for m in re.finditer(r"^\s+([a-z][a-z0-9_]+)\b", bodies.get(name, ""), re.M))
        out[name] = dict(ops=ops, vgpr=get("vgpr_count"), agpr=get("agpr_count"), sgpr=get("sgpr_count"), vspill=get("vgpr_spill_count"), sspill=get("sgpr_spill_count"),
                         scratch=get("private_segment_fixed_size"), lds=get("group_segment_fixed_size"), kernarg=get("kernarg_segment_size"))
    return out


def demangle(names):
    try:
        res = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
        return dict(zip(names, (re.sub(r"\((?!anonymous).*", "", r).replace("void ", "").replace("ncsn::", "") for r in res)))
    except Exception:
        return {n: n for n in names}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("this")
    ap.add_argument("--match", default=STREAM_WRITERS)
    ap.add_argument("--also", default=None)
    a = ap.parse_args()
    A, B = parse(a.parent), parse(a.this)
    nice = demangle(sorted(set(A) | set(B)))
    if a.also:
        C = parse(a.also)
        nice_c = demangle(sorted(C))
        have = {re.sub(r"\(anonymous namespace\)::", "", v) for v in nice.values()}
        dup = [n for n in C if re.sub(r"\(anonymous namespace\)::", "", nice_c[n]) in have]
        print(f"{a.also.split('/')[-1].split('-')[0]}: {len(C)} kernels, {len(dup)} of them the shared headers' non-template kernels that {a.this.split('/')[-1].split('-')[0]} holds too (internal linkage, no caller here)")
        B.update({n: v for n, v in C.items() if n not in dup})
    gone, new = sorted(set(A) - set(B)), sorted(set(B) - set(A))
    nice = demangle(sorted(set(A) | set(B)))
    nice = {k: v.replace("(anonymous namespace)::", "") for k, v in nice.items()}
    print(f"kernel symbols: parent {len(A)}, this build {len(B)}; in the parent only: {len(gone)}; new: {len(new)}")
    for n in gone:
        print("  MISSING  " + nice[n])
    for n in new:
        print("  new      " + nice[n])
    same_all = [n for n in A if n in B and A[n]["ops"] == B[n]["ops"] and all(A[n][k] == B[n][k] for k in ("vgpr", "agpr", "sgpr", "vspill", "sspill", "scratch", "lds"))]
    print(f"kernels of both builds with identical opcode counts, registers, spills, scratch and LDS: {len(same_all)} of {len(set(A) & set(B))}")
    for n in sorted(set(A) & set(B)):
        if n not in same_all:
            d = {k: (A[n]["ops"][k], B[n]["ops"][k]) for k in set(A[n]["ops"]) | set(B[n]["ops"]) if A[n]["ops"][k] != B[n]["ops"][k]}
            r = {k: (A[n][k], B[n][k]) for k in ("vgpr", "agpr", "sgpr", "vspill", "sspill", "scratch", "lds") if A[n][k] != B[n][k]}
            print(f"  DIFFERS  {nice[n]}: opcodes {d} registers {r}")
    print()
    print("stream-writing instances (parent -> this build; '=' when equal; guarded instances exist in this build only)")
    print(f"{'kernel':58s} {'instr':>15s} {'opcode kinds':>12s} {'VGPR':>10s} {'AGPR':>10s} {'SGPR':>10s} {'spill v/s, scratch':>18s} {'kernarg':>10s} atomics")
    for n in sorted(set(A) | set(B), key=lambda n: nice[n]):
        if not re.search(a.match, n):
            continue
        x, y = A.get(n), B.get(n)

        def col(f, w):
            va, vb = (f(x) if x else None), (f(y) if y else None)
            s = f"{vb}" if va is None else (f"{va} =" if va == vb else f"{va} -> {vb}")
            return s.rjust(w)
        z = y or x
        atom = {k: v for k, v in z["ops"].items() if "atomic" in k}
        eq = "" if not (x and y) else ("  opcode counts equal" if x["ops"] == y["ops"] else "  OPCODE COUNTS DIFFER")
        print(f"{nice[n][:58]:58s} {col(lambda k: sum(k['ops'].values()), 15)} {col(lambda k: len(k['ops']), 12)} {col(lambda k: k['vgpr'], 10)} {col(lambda k: k['agpr'], 10)} "
              f"{col(lambda k: k['sgpr'], 10)} {col(lambda k: (k['vspill'], k['sspill'], k['scratch']), 18)} {col(lambda k: k['kernarg'], 10)} {atom or '-'}{eq}")


if __name__ == "__main__":
    main()
