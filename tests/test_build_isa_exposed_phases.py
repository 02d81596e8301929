"""The exposed phases of the fused-convolution tiles, counted on the built listings (tools/exposed_phase_census.py; profiles/r08/exposed_phase_census.txt holds the table of
the commit before round 8 and of this tree): what runs in front of the first and behind the last `v_mfma` of a tile has no matrix work under it, so an instruction there is
paid in full.  Round 8 took two pieces of work out that the result does not need:

  * k_conv_gn3 zeroed its 256 accumulator registers TWICE (hipcc re-materialised the constant tile on both sides of the K loop's guard: 512 writes in front of the loop);
  * the packed epilogue's GroupNorm partial sums were scalar (3 + 1 adds and a packed square + 3 + 1 adds per four values); they are packed fp32 pairs now.

The bounds are the ones the round set itself from the parent's counts (1,791 / 1,796 / 1,924 vector instructions behind the last MFMA of k_conv_gn3<*, *, *, 2> with 504 / 505
`v_add_f32`; 813 / 827 for k_conv_gn2<32, false, 2, 8, 1, 4> / k_conv_gn_upfold<2>): a compiler or source change that brings the work back fails here."""
import importlib.util
import re
from pathlib import Path

import pytest

import test_build_isa as isa
from test_build_isa import listings  # noqa: F401  (the fixture: builds when out of date, reads the listings)

_spec = importlib.util.spec_from_file_location("exposed_phase_census", Path(__file__).resolve().parent.parent / "tools" / "exposed_phase_census.py")
census = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(census)

# vector instructions behind the last v_mfma in the commit before round 8 (profiles/r08/exposed_phase_census.txt)
PARENT_EPILOGUE = {
    "ncsn::k_conv_gn3<32, 4, 1, 2>": 1791, "ncsn::k_conv_gn3<32, 2, 2, 2>": 1796, "ncsn::k_conv_gn3<16, 2, 2, 2>": 1924,
    "ncsn::k_conv_gn2<32, false, 2, 8, 1, 4>": 813, "ncsn::k_conv_gn_upfold<2>": 827,
}


@pytest.fixture(scope="module")
def phases(listings):  # noqa: F811
    return census.census(isa.BUILD)          # (conv_gn3, ncsnpp and up_fold: the fixture above has built them)


def test_the_census_sees_the_kernels_the_metadata_lists(listings, phases):  # noqa: F811
    """same parsing as tests/test_build_isa.py: every k_conv_gn3 / k_conv_gn2 / k_conv_gn_upfold kernel of the code objects' metadata has its two phases"""
    want = {re.sub(r"^void |\(.*$", "", n.replace("(anonymous namespace)::", ""))
            for stem in census.UNITS for n in isa._kernels((isa.BUILD / f"{stem}-hip-amdgcn-amd-amdhsa-gfx950.s").read_text()) if any(k in n for k in census.KERNELS)}
    assert want == set(phases) and sum("k_conv_gn3" in n for n in want) == 12, sorted(want ^ set(phases))


def test_conv_gn3_zeroes_its_accumulators_once(phases):
    """at most 256 + 8 accumulator registers are set to zero in front of the first MFMA (the parent: 512 `v_accvgpr_write_b32 aN, 0`), whichever form hipcc gives the
    write -- an inline 0 or a copy of an accumulator that holds one -- and no register twice"""
    seen = 0
    for name, ph in phases.items():
        if "k_conv_gn3" not in name:
            continue
        pro = ph["prologue"]
        zero = census.zeroed(pro)
        assert len(zero) <= 256 + 8, (name, len(zero))
        init = [i for i in pro if i[0] in ("v_accvgpr_write_b32", "v_accvgpr_mov_b32")]
        dst = [re.match(r"\S+\s+(a\d+),", ln).group(1) for _, ln in init]
        assert len(init) <= 256 + 8 and len(set(dst)) == len(dst), (name, len(init), len(set(dst)))
        seen += 1
    assert seen == 12


def test_conv_gn3_epilogue_sums_are_packed(phases):
    for name in ("ncsn::k_conv_gn3<32, 4, 1, 2>", "ncsn::k_conv_gn3<32, 2, 2, 2>", "ncsn::k_conv_gn3<16, 2, 2, 2>"):
        v = census.vector(phases[name]["epilogue"])
        adds = sum(op.startswith("v_add_f32") and "dpp" not in op for op, _ in v)
        assert adds <= 200, (name, adds)
        assert len(v) <= PARENT_EPILOGUE[name] - 300, (name, len(v))


def test_conv_gn2_and_upfold_epilogues_shrink_with_it(phases):
    for name in ("ncsn::k_conv_gn2<32, false, 2, 8, 1, 4>", "ncsn::k_conv_gn_upfold<2>"):
        v = census.vector(phases[name]["epilogue"])
        assert len(v) <= PARENT_EPILOGUE[name] - 150, (name, len(v))
