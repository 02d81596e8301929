"""ISA check of the x0-projection kernels of the CIFAR10 form (csrc/ni_step.hip, k_x0project_f64 and k_stepproject_f64, one instantiation per LDS
capacity) in the listing `make` leaves in csrc/build/ (-save-temps=obj): they fit their registers -- no VGPR or SGPR spills, no scratch memory;
every output is stored once; and the projection on its own, which holds no division, holds no fused multiply-add."""
import re
import subprocess
from pathlib import Path

import pytest

CSRC = Path(__file__).resolve().parent.parent / "naturaldiffusion_amd" / "csrc"
LISTING = CSRC / "build" / "ni_step-hip-amdgcn-amd-amdhsa-gfx950.s"


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


@pytest.mark.parametrize("kernel", ["k_x0project_f64", "k_stepproject_f64"])
def test_projection_kernels_fit_their_registers_and_store_each_output_once(listing, kernel):
    found = _kernels(listing, kernel)
    assert len(found) == 2, [f[0] for f in found]                                            # 768 quads (32x32x3) and 2,048 quads (the cap)
    for name, vs, ss, scratch, group, ops in found:
        assert vs == 0 and ss == 0 and scratch == 0, (name, vs, ss, scratch)
        stores = [o for o in ops if o.startswith(("global_store", "flat_store", "buffer_store", "scratch_store"))]
        # k_x0project_f64: the projected quad (two 16-byte stores) + r_out; k_stepproject_f64: hist[k] (two) + x_next (one) + r_out -- the raw x0 is never stored
        assert stores.count("global_store_dwordx4") == (2 if kernel == "k_x0project_f64" else 3), (name, stores)
        assert stores.count("global_store_dwordx2") == 1 and len(stores) == stores.count("global_store_dwordx4") + 1, (name, stores)
        if kernel == "k_x0project_f64":
            assert not [o for o in ops if o.startswith("v_fma_f64")], name
