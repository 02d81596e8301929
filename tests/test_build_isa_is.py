"""ISA check of the Inception Score's kernels (csrc/prdc.h: k_is_logits, k_is_rows) in the listing `make` leaves in csrc/build/ (-save-temps=obj): they
exist, fit their registers -- no spills, no scratch memory --, the logit sweep runs on bf16 MFMAs only and two of its blocks fit a CU's registers and LDS."""
import pytest

from test_build_isa_kid import CSRC, LDS_PER_CU, _kernel, listing  # noqa: F401  (the same listing, read the same way)

KERNELS = ["k_is_logits", "k_is_rows"]


def test_the_unit_compiles_without_a_warning(listing):
    assert (CSRC / "build" / "prdc.diag").read_text() == ""


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_spills_no_scratch(listing, kernel):
    name, get, ops = _kernel(listing, kernel)
    assert get("vgpr_spill_count") == 0 and get("sgpr_spill_count") == 0 and get("private_segment_fixed_size") == 0, name


def test_the_logit_sweep_runs_on_bf16_mfma_only(listing):
    name, get, ops = _kernel(listing, "k_is_logits")
    mfma = [o for o in ops if o.startswith("v_mfma")]
    # the distance kernels' K loop: 2 steps of 16 x 6 plane products x 2 accumulators per K tile of 32, every matrix instruction on bf16 operands
    assert len(mfma) >= 24 and set(mfma) == {"v_mfma_f32_32x32x16_bf16"}, (name, sorted(set(mfma)), len(mfma))
    assert get("vgpr_count") <= 256, (name, get("vgpr_count"))                               # two blocks of four waves per CU
    assert 2 * get("group_segment_fixed_size") <= LDS_PER_CU, (name, get("group_segment_fixed_size"))
