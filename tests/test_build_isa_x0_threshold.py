"""ISA check of the x0-correction kernels of the CIFAR10 form (csrc/ni_step.hip, k_x0fix_f64 and k_stepfix_f64, one instantiation per LDS
capacity) in the listing `make` leaves in csrc/build/ (-save-temps=obj): they fit their registers -- no VGPR or SGPR spills, no scratch memory;
the image and the search live in LDS, so there is no flat, buffer or global-atomic instruction (the histogram is LDS integer atomics); the
quantile's one fused multiply-add is there; and no name collides with a tag of test_build_isa.py's EXACT tuple, whose kernels may hold no
fused operation outside a division."""
import re
import subprocess
from pathlib import Path

import pytest

CSRC = Path(__file__).resolve().parent.parent / "naturaldiffusion_amd" / "csrc"
LISTING = CSRC / "build" / "ni_step-hip-amdgcn-amd-amdhsa-gfx950.s"
EXACT = ("k_step_f64hist", "k_wsum_f64", "k_step_f32prod", "k_wsum_f32prod", "k_flow_input_f16", "k_wmean_f16", "k_step_f16chain",
         "k_to_pixel")                                                    # tests/test_build_isa.py


def _kernels(text, kernel):
    """[(mangled name, vgpr spills, sgpr spills, scratch bytes, LDS bytes, instruction mnemonics in program order)] of every kernel whose name
    contains `kernel`"""
    md = text[text.index("amdhsa.kernels:"):]
    code = text[:text.index("amdhsa.kernels:")]
    found = []
    for blk in re.split(r"\n  - \.", md)[1:]:
        name = re.search(r"\.name:\s*(\S+)", blk).group(1)
        if kernel in name:
            get = lambda key: int(re.search(r"\." + key + r":\s*(\S+)", blk).group(1))
            body = code[code.index("\n" + name + ":"):]
            body = body[:body.index(".Lfunc_end")]
            found.append((name, get("vgpr_spill_count"), get("sgpr_spill_count"), get("private_segment_fixed_size"),
                          get("group_segment_fixed_size"), re.findall(r"^\s+([a-z]\w+)", body, flags=re.M)))
    return found


@pytest.fixture(scope="module")
def listing():
    subprocess.check_call(["make", "-C", str(CSRC), "-j4"], stdout=subprocess.DEVNULL)       # no-op when up to date
    return LISTING.read_text()


@pytest.mark.parametrize("kernel", ["k_x0fix_f64", "k_stepfix_f64"])
def test_correction_kernels_fit_their_registers_and_stay_in_lds(listing, kernel):
    found = _kernels(listing, kernel)
    assert len(found) == 2, [f[0] for f in found]                                            # 768 quads (32x32x3) and 2,048 quads (the cap)
    lds = []
    for name, vs, ss, scratch, group, ops in found:
        assert vs == 0 and ss == 0 and scratch == 0, (name, vs, ss, scratch)
        bad = [o for o in ops if o.startswith(("flat_", "buffer_", "scratch_", "global_atomic"))]
        assert not bad, (name, sorted(set(bad)))
        assert any(o.startswith("v_fma_f64") for o in ops), name
        assert any(o.startswith("ds_add_u32") for o in ops) and any(o.startswith("ds_min") for o in ops), name      # the histogram, the minimum above a[lo]
        assert not [o for o in ops if re.match(r"ds_\w*_f(32|64)", o) and ("add" in o or "min" in o or "max" in o)], name      # no float atomics
        assert not any(tag in name for tag in EXACT), name
        stores = [o for o in ops if o.startswith("global_store")]
        # k_x0fix_f64: the corrected quad (two 16-byte stores) + s_out; k_stepfix_f64: hist[k] (two) + x_next (one) + s_out -- the raw x0 is never stored
        assert stores.count("global_store_dwordx4") == (2 if kernel == "k_x0fix_f64" else 3), (name, stores)
        assert stores.count("global_store_dwordx2") == 1 and len(stores) == stores.count("global_store_dwordx4") + 1, (name, stores)
        lds.append(group)
    assert sorted(lds)[0] >= 768 * 32 and sorted(lds)[0] < 32 * 1024 and 2048 * 32 <= sorted(lds)[1] < 72 * 1024, lds
