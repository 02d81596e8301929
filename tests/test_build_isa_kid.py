"""ISA check of the kernel-distance kernels (csrc/prdc.h: k_kid_sums, k_kid_merge) in the listing `make` leaves in csrc/build/ (-save-temps=obj): they
exist, fit their registers -- no spills, no scratch memory --, the sweep runs on bf16 MFMAs only and two of its blocks fit a CU's registers and LDS."""
import re
import subprocess
from pathlib import Path

import pytest

CSRC = Path(__file__).resolve().parent.parent / "naturaldiffusion_amd" / "csrc"
KERNELS = ["k_kid_sums", "k_kid_merge"]
LDS_PER_CU = 160 * 1024


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
def listing():
    subprocess.check_call(["make", "-C", str(CSRC), "-j4"], stdout=subprocess.DEVNULL)       # no-op when up to date
    return (CSRC / "build" / "prdc-hip-amdgcn-amd-amdhsa-gfx950.s").read_text()


def test_the_unit_compiles_without_a_warning(listing):
    assert (CSRC / "build" / "prdc.diag").read_text() == ""


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_spills_no_scratch(listing, kernel):
    name, get, ops = _kernel(listing, kernel)
    assert get("vgpr_spill_count") == 0 and get("sgpr_spill_count") == 0 and get("private_segment_fixed_size") == 0, name
    assert not [o for o in ops if o.startswith(("scratch_", "flat_", "buffer_"))], (name, sorted(set(ops)))


def test_the_sweep_runs_on_bf16_mfma_only(listing):
    name, get, ops = _kernel(listing, "k_kid_sums")
    mfma = [o for o in ops if o.startswith("v_mfma")]
    # the distance kernels' K loop: 2 steps of 16 x 6 plane products x 2 accumulators per K tile of 32, every matrix instruction on bf16 operands
    assert len(mfma) >= 24 and set(mfma) == {"v_mfma_f32_32x32x16_bf16"}, (name, sorted(set(mfma)), len(mfma))
    assert get("vgpr_count") <= 256, (name, get("vgpr_count"))                               # two blocks of four waves per CU
    assert 2 * get("group_segment_fixed_size") <= LDS_PER_CU, (name, get("group_segment_fixed_size"))
    assert ops.count("global_load_dwordx4") >= 9 and {o for o in ops if o.startswith("global_load")} == {"global_load_dwordx4"}, name    # no norms, no radii
    # the epilogue is fp64: u = gamma s + coef0 (a multiply-add or a multiply and an add), two multiplies for the cube, one add into the row's sum, 32 times
    assert ops.count("v_mul_f64") >= 64 and ops.count("v_fma_f64") + ops.count("v_add_f64") >= 96, name
    assert not [o for o in ops if "atomic" in o], name                                       # a sum in a fixed order


def test_the_merge_adds_in_a_loop_without_atomics(listing):
    name, get, ops = _kernel(listing, "k_kid_merge")
    assert "v_add_f64" in ops and not [o for o in ops if "atomic" in o], name
    assert {o for o in ops if o.startswith("global_store")} == {"global_store_dwordx2"}, name
