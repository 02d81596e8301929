"""Static census of the exposed phases of the fused-convolution kernels: the instructions in front of the first and behind the last `v_mfma` of every k_conv_gn3 /
k_conv_gn2 / k_conv_gn_upfold kernel in the listings a build leaves in csrc/build/ (profiles/r08/exposed_phase_census.txt; tests/test_build_isa_exposed_phases.py
asserts on the same counts).  A phase is counted in LISTING order: the prologue holds every path in front of the K loop, taken or not.
usage: exposed_phase_census.py [build directory] [label]"""
import re
import subprocess
import sys
from collections import Counter
from pathlib import Path

BUILD = Path(__file__).resolve().parent.parent / "naturaldiffusion_amd" / "csrc" / "build"
KERNELS = ("k_conv_gn3", "k_conv_gn2", "k_conv_gn_upfold")
UNITS = ("conv_gn3", "ncsnpp", "up_fold")          # the translation units that hold them
ZERO_ACC = re.compile(r"v_accvgpr_write_b32\s+a\d+,\s*0\s*(;.*)?$")


def instructions(body):
    """[(mnemonic, whole line)] of a function body: labels, directives and comment lines left out"""
    out = []
    for ln in body.split("\n"):
        s = ln.strip()
        if not s or s.startswith((";", ".")) or re.match(r"^[\w.$]+:", s):
            continue
        out.append((s.split()[0], s))
    return out


def phases(listing):
    """demangled kernel name -> dict(prologue=[...], epilogue=[...]) of (mnemonic, line) lists, for the fused-convolution kernels of one listing"""
    code = listing[:listing.index("amdhsa.kernels:")] if "amdhsa.kernels:" in listing else listing
    found = []
    for m in re.finditer(r"^(_Z\w+):\s*; @", code, flags=re.M):
        if not any(k in m.group(1) for k in KERNELS):
            continue
        end = re.compile(r"^\.Lfunc_end\d+:", flags=re.M).search(code, m.end()).start()
        ins = instructions(code[m.end():end])
        at = [i for i, (op, _) in enumerate(ins) if op.startswith("v_mfma")]
        if at:
            found.append((m.group(1), ins[:at[0]], ins[at[-1] + 1:]))
    if not found:
        return {}
    names = subprocess.run(["c++filt"] + [f[0] for f in found], capture_output=True, text=True, check=True).stdout.strip().split("\n")
    return {re.sub(r"^void |\(.*$", "", n.replace("(anonymous namespace)::", "")): dict(prologue=p, epilogue=e) for n, (_, p, e) in zip(names, found)}


def vector(ins):
    return [i for i in ins if i[0].startswith("v_")]


def zeroed(ins):
    """accumulator registers written with an inline 0"""
    return [i for i in ins if ZERO_ACC.match(i[1])]


def census(build=BUILD):
    out = {}
    for stem in UNITS:
        out.update(phases((Path(build) / f"{stem}-hip-amdgcn-amd-amdhsa-gfx950.s").read_text()))
    return out


def main():
    build = Path(sys.argv[1]) if len(sys.argv) > 1 else BUILD
    label = sys.argv[2] if len(sys.argv) > 2 else str(build)
    print(f"# {label}: instructions in front of the first / behind the last v_mfma, in listing order")
    print(f"{'kernel':<58} {'phase':<9} {'vector':>6} {'acc=0':>6}  of which")
    for name, ph in sorted(census(build).items()):
        for which in ("prologue", "epilogue"):
            v = vector(ph[which])
            top = Counter(op for op, _ in v).most_common(7)
            print(f"{name:<58} {which:<9} {len(v):6d} {len(zeroed(ph[which])):6d}  " + ", ".join(f"{n} {op}" for op, n in top))


if __name__ == "__main__":
    main()
