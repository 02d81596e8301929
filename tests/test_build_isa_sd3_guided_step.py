"""ISA check of the SD3-form step with per-image guidance (csrc/ni_step.hip, k_step_f16chain_guided) in the listing `make` leaves in
csrc/build/ (-save-temps=obj): two instances, one per NATINF_SD3_CFG_ON_VELOCITY value; each fits its registers -- no VGPR or SGPR spills, no
scratch memory; and its streams are 16-byte accesses -- x, v_text, v_null, the noise and the history rows are read, hist[k], mean_out and x_next
written, as dwordx4, with the two per-image values (scale, slot) the only single-dword loads."""
import re
import subprocess
from pathlib import Path

CSRC = Path(__file__).resolve().parent.parent / "naturaldiffusion_amd" / "csrc"
LISTING = CSRC / "build" / "ni_step-hip-amdgcn-amd-amdhsa-gfx950.s"
KERNEL = "k_step_f16chain_guided"


def test_sd3_guided_step_two_instances_without_spills_or_scratch_and_streams_16_bytes():
    subprocess.check_call(["make", "-C", str(CSRC), "-j4"], stdout=subprocess.DEVNULL)       # no-op when up to date
    text = LISTING.read_text()
    md = text[text.index("amdhsa.kernels:"):]
    found = {}
    for blk in re.split(r"\n  - \.", md)[1:]:
        name = re.search(r"\.name:\s*(\S+)", blk).group(1)
        if KERNEL in name:
            get = lambda key: int(re.search(r"\." + key + r":\s*(\S+)", blk).group(1))
            found[name] = (get("vgpr_spill_count"), get("sgpr_spill_count"), get("private_segment_fixed_size"))
    assert len(found) == 2, found                                                        # <false> and <true>
    assert sorted("ILb1E" in name for name in found) == [False, True], found
    code = text[:text.index("amdhsa.kernels:")]
    for name, (vs, ss, scratch) in found.items():
        assert vs == 0 and ss == 0 and scratch == 0, (name, vs, ss, scratch)
        # the kernel's code: from its label to the end of the function
        body = code[code.index("\n" + name + ":"):]
        body = body[:body.index(".Lfunc_end")]
        ops = re.findall(r"^\s+((?:global|flat|scratch|buffer)_\w+)", body, flags=re.M)
        assert not [o for o in ops if o.startswith(("scratch_", "flat_", "buffer_"))], (name, sorted(set(ops)))
        stores = [o for o in ops if "_store_" in o]
        assert stores == ["global_store_dwordx4"] * 3, (name, stores)                    # hist[k], mean_out and x_next, nothing narrower
        loads = [o for o in ops if "_load_" in o]
        # x, v_text, v_null, noise, and the history rows (the term loop unrolled by 4, and its remainder): every one a 16-byte load
        assert loads.count("global_load_dwordx4") >= 5, (name, loads)
        # what else is loaded per thread: cfg_image[img] and uncond_slot[img], one dword each
        rest = sorted(o for o in loads if o != "global_load_dwordx4")
        assert rest == ["global_load_dword", "global_load_dword"], (name, rest)
