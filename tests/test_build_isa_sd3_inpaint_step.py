"""ISA check of the inpainting step of the SD3 form (csrc/ni_step.hip, k_step_inpaint_f16chain) in the listing `make` leaves in csrc/build/
(-save-temps=obj): two instances, one per NATINF_SD3_CFG_ON_VELOCITY value; each fits its registers -- no VGPR or SGPR spills, no scratch memory;
hist[k], mean_out and x_next leave in one 16-byte store each, x_next after the blend; every stream is a 16-byte load, the mask word and the int64
global index the 8-byte loads, the image's scale and slot the single-dword loads."""
import re
import subprocess
from pathlib import Path

import pytest

CSRC = Path(__file__).resolve().parent.parent / "naturaldiffusion_amd" / "csrc"
LISTING = CSRC / "build" / "ni_step-hip-amdgcn-amd-amdhsa-gfx950.s"
KERNEL = "k_step_inpaint_f16chain"


def _kernels(text, kernel):
    """[(mangled name, vgpr spills, sgpr spills, scratch bytes)] of every kernel whose name contains `kernel`"""
    md = text[text.index("amdhsa.kernels:"):]
    found = []
    for blk in re.split(r"\n  - \.", md)[1:]:
        name = re.search(r"\.name:\s*(\S+)", blk).group(1)
        if kernel in name:
            get = lambda key: int(re.search(r"\." + key + r":\s*(\S+)", blk).group(1))
            found.append((name, get("vgpr_spill_count"), get("sgpr_spill_count"), get("private_segment_fixed_size")))
    return found


def _memory_ops(text, name):
    """the memory mnemonics of kernel `name` in program order"""
    code = text[:text.index("amdhsa.kernels:")]
    body = code[code.index("\n" + name + ":"):]
    body = body[:body.index(".Lfunc_end")]
    return re.findall(r"^\s+((?:global|flat|scratch|buffer)_\w+)", body, flags=re.M)


@pytest.fixture(scope="module")
def listing():
    subprocess.check_call(["make", "-C", str(CSRC), "-j4"], stdout=subprocess.DEVNULL)       # no-op when up to date
    return LISTING.read_text()


def test_two_instances_whose_names_collide_with_no_other_selection(listing):
    found = _kernels(listing, KERNEL)
    assert len(found) == 2, found                                                            # <false> and <true>
    assert sorted("ILb1E" in name for name, *_ in found) == [False, True], found
    # the substrings the other ISA tests select by still select what they selected: none of them matches the new kernels
    for other, count in (("k_step_f16chain_guided", 2), ("k_step_f16chain", 4), ("k_known_blend", 1), ("k_step_inpaint_f64", 1),
                         ("k_step_inpaint_f32prod", 1), ("k_flow_input_f16", 1)):
        for name, *_ in found:
            assert other not in name, (other, name)
        assert len(_kernels(listing, other)) == count, other
    # the blend on its own: one kernel, and not one "k_known_blend" selects
    (blend, vs, ss, scratch), = _kernels(listing, "k_blend_known_f16")
    assert vs == 0 and ss == 0 and scratch == 0 and "k_known_blend" not in blend


@pytest.mark.parametrize("velocity", [False, True])
def test_no_spills_no_scratch_three_16_byte_stores(listing, velocity):
    (name, vs, ss, scratch), = [f for f in _kernels(listing, KERNEL) if ("ILb1E" in f[0]) == velocity]
    assert vs == 0 and ss == 0 and scratch == 0, (name, vs, ss, scratch)
    ops = _memory_ops(listing, name)
    assert not [o for o in ops if o.startswith(("scratch_", "flat_", "buffer_"))], (name, sorted(set(ops)))
    # hist[k], mean_out and x_next: 16 bytes each, and x_next is stored once -- the blend happens in registers in front of it
    stores = [o for o in ops if "_store_" in o]
    assert stores == ["global_store_dwordx4"] * 3, (name, stores)
    loads = [o for o in ops if "_load_" in o]
    assert loads.count("global_load_dword") == 2, (name, loads)                              # cfg_image[img], uncond_slot[img]
    assert loads.count("global_load_dwordx2") == 2, (name, loads)                            # the mask word, the int64 global index
    # x, v_text, v_null, noise, known (the next input's and the mean's) and the history rows: every stream a 16-byte load
    assert sorted(set(loads)) == ["global_load_dword", "global_load_dwordx2", "global_load_dwordx4"], (name, sorted(set(loads)))
    assert loads.count("global_load_dwordx4") >= 6, (name, loads)
