"""ISA check of the posterior statistics' kernels in the listings `make` leaves in csrc/build/ (-save-temps=obj): k_post_samples (csrc/ni_step.hip) and
k_post_norms / k_post_dots / k_post_rows (csrc/posterior.hip) fit their registers -- no VGPR or SGPR spills, no scratch memory; the GEMM runs on bf16 MFMAs only,
two blocks to a CU; the sample kernel moves its data in 16-byte accesses only."""
import re
import subprocess
from pathlib import Path

import pytest

CSRC = Path(__file__).resolve().parent.parent / "naturaldiffusion_amd" / "csrc"


def _kernel(text, kernel):
    """(mangled name, metadata getter, instruction mnemonics in program order) of the one kernel whose name contains `kernel`"""
    md = text[text.index("amdhsa.kernels:"):]
    found = []
    for blk in re.split(r"\n  - \.", md)[1:]:
        name = re.search(r"\.name:\s*(\S+)", blk).group(1)
        if kernel in name:
            found.append((name, blk))
    assert len(found) == 1, [f[0] for f in found]
    name, blk = found[0]
    get = lambda key: int(re.search(r"\." + key + r":\s*(\S+)", blk).group(1))
    code = text[:text.index("amdhsa.kernels:")]
    body = code[code.index("\n" + name + ":"):]
    body = body[:body.index(".Lfunc_end")]
    return name, get, re.findall(r"^\s+([a-z]\w+)", body, flags=re.M)


@pytest.fixture(scope="module")
def listings():
    subprocess.check_call(["make", "-C", str(CSRC), "-j4"], stdout=subprocess.DEVNULL)       # no-op when up to date
    return {u: (CSRC / "build" / f"{u}-hip-amdgcn-amd-amdhsa-gfx950.s").read_text() for u in ("ni_step", "posterior")}


@pytest.mark.parametrize("unit,kernel", [("ni_step", "k_post_samples"), ("posterior", "k_post_norms"), ("posterior", "k_post_dots"), ("posterior", "k_post_rows")])
def test_no_spills_no_scratch(listings, unit, kernel):
    name, get, ops = _kernel(listings[unit], kernel)
    assert get("vgpr_spill_count") == 0 and get("sgpr_spill_count") == 0 and get("private_segment_fixed_size") == 0, name
    assert not [o for o in ops if o.startswith(("scratch_", "flat_", "buffer_"))], (name, sorted(set(ops)))


def test_dots_runs_on_bf16_mfma_only(listings):
    name, get, ops = _kernel(listings["posterior"], "k_post_dots")
    mfma = [o for o in ops if o.startswith("v_mfma")]
    # one K tile: 4 steps of 16 x 3 planes x 2 accumulators; every matrix instruction takes bf16 operands (an f32-input MFMA runs at 1/16 of the rate)
    assert len(mfma) == 24 and set(mfma) == {"v_mfma_f32_32x32x16_bf16"}, (name, sorted(set(mfma)), len(mfma))
    assert get("vgpr_count") <= 256, (name, get("vgpr_count"))                               # two blocks of four waves per CU
    assert get("group_segment_fixed_size") <= 80 * 1024, name                                # ... and their LDS beside each other
    # operands and fragments move 16 bytes at a time; the fp64 partial sums leave as 8-byte stores, 32 consecutive ones per instruction
    assert {o for o in ops if o.startswith("global_load")} == {"global_load_dwordx4"}
    assert {o for o in ops if o.startswith("ds_")} == {"ds_write_b128", "ds_read_b128"}
    assert {o for o in ops if o.startswith("global_store")} == {"global_store_dwordx2"}
    assert ops.count("v_add_f64") == 32, name                                                # the fp64 accumulators: one add per output element and flush


def test_samples_moves_16_bytes_at_a_time(listings):
    name, get, ops = _kernel(listings["ni_step"], "k_post_samples")
    mem = [o for o in ops if o.startswith(("global_", "flat_", "scratch_", "buffer_"))]
    assert sorted(mem) == ["global_load_dwordx4"] * 3 + ["global_store_dwordx4"] * 3, (name, mem)      # f and two noise quads in, three planes out
    assert ops.count("v_cvt_pk_bf16_f32") == 12, name                                        # 3 planes x 8 values, round to nearest even in hardware
