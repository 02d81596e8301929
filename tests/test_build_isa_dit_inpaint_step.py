"""ISA check of the inpainting step of the Validate form (csrc/ni_step.hip, k_step_inpaint_f32prod) in the listing `make` leaves in csrc/build/
(-save-temps=obj): it fits its registers -- no VGPR or SGPR spills, no scratch memory; hist_x0[k] and z_next leave in one 16-byte store each, z_next
after the blend; the only single-dword loads are the image's scale, its slot and the mask word of the quad; every stream is a 16-byte load and the
int64 global index the one 8-byte load."""
import re
import subprocess
from pathlib import Path

import pytest

CSRC = Path(__file__).resolve().parent.parent / "naturaldiffusion_amd" / "csrc"
LISTING = CSRC / "build" / "ni_step-hip-amdgcn-amd-amdhsa-gfx950.s"
KERNEL = "k_step_inpaint_f32prod"


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


def test_the_kernel_exists_exactly_once(listing):
    found = _kernels(listing, KERNEL)
    assert len(found) == 1, found
    # and its name collides with none of the substrings the other ISA tests select by
    for other in ("k_step_guided_f32prod", "k_step_noise_f32prod", "k_step_inpaint_f64", "k_known_blend"):
        assert other not in found[0][0]
        assert len(_kernels(listing, other)) == 1, other


def test_no_spills_no_scratch_two_16_byte_stores_three_dword_loads(listing):
    (name, vs, ss, scratch), = _kernels(listing, KERNEL)
    assert vs == 0 and ss == 0 and scratch == 0, (name, vs, ss, scratch)
    ops = _memory_ops(listing, name)
    assert not [o for o in ops if o.startswith(("scratch_", "flat_", "buffer_"))], (name, sorted(set(ops)))
    # hist_x0[k] and z_next: 16 bytes each, and z_next is stored once -- the blend happens in registers in front of it
    stores = [o for o in ops if "_store_" in o]
    assert stores == ["global_store_dwordx4"] * 2, (name, stores)
    loads = [o for o in ops if "_load_" in o]
    assert loads.count("global_load_dword") == 3, (name, loads)                              # cfg_image[img], uncond_slot[img], the mask word
    # z, cond, uncond, eps_0, known and the history rows: every stream a 16-byte load; the int64 global index the one 8-byte load
    rest = sorted(set(loads) - {"global_load_dword", "global_load_dwordx4"})
    assert rest in ([], ["global_load_dwordx2"]), (name, rest)
    assert loads.count("global_load_dwordx2") <= 1, (name, loads)
    assert loads.count("global_load_dwordx4") >= 6, (name, loads)
