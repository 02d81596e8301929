"""ISA check of the manifold-metric kernels (csrc/prdc.hip) in the listing `make` leaves in csrc/build/ (-save-temps=obj): the kernels exist, fit their
registers -- no spills, no scratch memory --, the three distance kernels run on bf16 MFMAs only with fp64 adds behind them, and two blocks fit a CU's LDS."""
import re
import subprocess
from pathlib import Path

import pytest

CSRC = Path(__file__).resolve().parent.parent / "naturaldiffusion_amd" / "csrc"
KERNELS = ["k_prdc_planes", "k_prdc_knn", "k_prdc_merge", "k_prdc_balls", "k_prdc_dist2"]
TILE_KERNELS = ["k_prdc_knn", "k_prdc_balls", "k_prdc_dist2"]
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


def test_the_unit_compiles_without_a_warning():
    subprocess.check_call(["make", "-C", str(CSRC), "-j4"], stdout=subprocess.DEVNULL)
    assert (CSRC / "build" / "prdc.diag").read_text() == ""


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_spills_no_scratch(listing, kernel):
    name, get, ops = _kernel(listing, kernel)
    assert get("vgpr_spill_count") == 0 and get("sgpr_spill_count") == 0 and get("private_segment_fixed_size") == 0, name
    assert not [o for o in ops if o.startswith(("scratch_", "flat_", "buffer_"))], (name, sorted(set(ops)))


@pytest.mark.parametrize("kernel", TILE_KERNELS)
def test_distances_run_on_bf16_mfma_only(listing, kernel):
    name, get, ops = _kernel(listing, kernel)
    mfma = [o for o in ops if o.startswith("v_mfma")]
    # one K tile of 32 is 2 steps of 16 x 6 plane products x 2 accumulators (more if the compiler unrolls K tiles); every matrix instruction takes bf16
    # operands (an f32-input MFMA runs at 1/16 of the rate)
    assert len(mfma) >= 24 and set(mfma) == {"v_mfma_f32_32x32x16_bf16"}, (name, sorted(set(mfma)), len(mfma))
    assert get("vgpr_count") <= 256, (name, get("vgpr_count"))                               # two blocks of four waves per CU
    assert 2 * get("group_segment_fixed_size") <= LDS_PER_CU, (name, get("group_segment_fixed_size"))      # ... and their LDS beside each other
    # operands and fragments move 16 bytes at a time: 3 + 6 chunks per K tile (the 8-byte loads are the norms and radii)
    assert ops.count("global_load_dwordx4") >= 9 and {o for o in ops if o.startswith("global_load")} <= {"global_load_dwordx4", "global_load_dwordx2"}, name
    assert {o for o in ops if o.startswith("ds_read_b128")} and {o for o in ops if o.startswith("ds_write_b128")}, name
    assert ops.count("v_add_f64") >= 32, name                                                # the fp64 accumulators: one add per output element and flush


def test_planes_round_in_hardware(listing):
    name, get, ops = _kernel(listing, "k_prdc_planes")
    assert ops.count("v_cvt_pk_bf16_f32") >= 12, name                                        # 3 planes x 8 values, round to nearest even
    assert {o for o in ops if o.startswith("global_store")} == {"global_store_dwordx4", "global_store_dwordx2"}, name


def test_balls_adds_integers_with_vector_atomics(listing):
    name, get, ops = _kernel(listing, "k_prdc_balls")
    assert [o for o in ops if o.startswith("global_atomic_add")], name
    assert not [o for o in ops if "atomic" in o and not o.startswith("global_atomic_add")], name
