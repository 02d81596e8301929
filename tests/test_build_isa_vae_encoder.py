"""ISA check of the AutoencoderKL encoder's three new kernels in the listings `make` leaves in csrc/build/ (-save-temps=obj): the posterior kernel
(csrc/ni_step.hip, k_vae_posterior), the input pass k_vae_images (csrc/vae_engine.inc, compiled in ncsnpp.hip) and the 1x1 quant_conv k_vae_quant (csrc/vae_quant.hip) fit
their registers -- no VGPR or SGPR spills, no scratch memory; the posterior leaves its latents, and the input pass its 64-channel pixels, as 16-byte stores only."""
import re
import subprocess
from pathlib import Path

import pytest

CSRC = Path(__file__).resolve().parent.parent / "naturaldiffusion_amd" / "csrc"


def _kernel(text, kernel):
    """(mangled name, vgpr spills, sgpr spills, scratch bytes, memory mnemonics in program order) of the one kernel whose name contains `kernel`"""
    md = text[text.index("amdhsa.kernels:"):]
    found = []
    for blk in re.split(r"\n  - \.", md)[1:]:
        name = re.search(r"\.name:\s*(\S+)", blk).group(1)
        if kernel in name:
            get = lambda key: int(re.search(r"\." + key + r":\s*(\S+)", blk).group(1))
            found.append((name, get("vgpr_spill_count"), get("sgpr_spill_count"), get("private_segment_fixed_size")))
    assert len(found) == 1, found
    name, vs, ss, scratch = found[0]
    code = text[:text.index("amdhsa.kernels:")]
    body = code[code.index("\n" + name + ":"):]
    body = body[:body.index(".Lfunc_end")]
    return name, vs, ss, scratch, re.findall(r"^\s+((?:global|flat|scratch|buffer)_\w+)", body, flags=re.M)


@pytest.fixture(scope="module")
def listings():
    subprocess.check_call(["make", "-C", str(CSRC), "-j4"], stdout=subprocess.DEVNULL)       # no-op when up to date
    return {u: (CSRC / "build" / f"{u}-hip-amdgcn-amd-amdhsa-gfx950.s").read_text() for u in ("ni_step", "ncsnpp", "vae_quant")}


def test_posterior_without_spills_or_scratch_16_byte_stores_only(listings):
    name, vs, ss, scratch, ops = _kernel(listings["ni_step"], "k_vae_posterior")
    assert vs == 0 and ss == 0 and scratch == 0, (name, vs, ss, scratch)
    assert not [o for o in ops if o.startswith(("scratch_", "flat_", "buffer_"))], (name, sorted(set(ops)))
    stores = [o for o in ops if "_store_" in o]
    assert stores and set(stores) == {"global_store_dwordx4"}, (name, stores)
    # the mean and the logvar quad: 16-byte loads; the int64 global index the one 8-byte load
    loads = [o for o in ops if "_load_" in o]
    assert loads.count("global_load_dwordx4") >= 2 and set(loads) <= {"global_load_dwordx4", "global_load_dwordx2"}, (name, loads)


def test_input_pass_without_spills_or_scratch_16_byte_stores_only(listings):
    name, vs, ss, scratch, ops = _kernel(listings["ncsnpp"], "k_vae_images")
    assert vs == 0 and ss == 0 and scratch == 0, (name, vs, ss, scratch)
    assert not [o for o in ops if o.startswith(("scratch_", "flat_", "buffer_"))], (name, sorted(set(ops)))
    stores = [o for o in ops if "_store_" in o]
    assert len(stores) == 8 and set(stores) == {"global_store_dwordx4"}, (name, stores)       # the 128 bytes of a pixel's 64 channels
    assert [o for o in ops if "_load_" in o] == ["global_load_dword"] * 3, (name, ops)         # one value of each colour plane


def test_quant_conv_without_spills_or_scratch(listings):
    name, vs, ss, scratch, ops = _kernel(listings["vae_quant"], "k_vae_quant")
    assert vs == 0 and ss == 0 and scratch == 0, (name, vs, ss, scratch)
    assert not [o for o in ops if o.startswith(("scratch_", "flat_", "buffer_"))], (name, sorted(set(ops)))
