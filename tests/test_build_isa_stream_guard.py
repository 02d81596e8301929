"""ISA check of the stream guard (NATINF_DIT_STREAM_GUARD; csrc/ncsnpp_kernels.h stream_guard_value / stream_guard_commit) in the gfx950 listing `make` leaves in
csrc/build/ (-save-temps=obj): every stream-writing epilogue has its guarded instance (csrc/stream_guard.hip, a translation unit of its own) beside the unguarded one
(ncsnpp.hip); a guarded instance reports through VECTOR atomics
on global memory -- one unsigned max, one add, and no atomic of any other kind -- clamps with v_med3_f32 and stores what its unguarded twin stores; it fits its
registers like that twin; and the unguarded twin holds no atomic at all (profiles/stream_guard/listing_ab.txt compares those twins with the parent commit's, opcode by opcode)."""
import re
import subprocess
from collections import Counter
from pathlib import Path

import pytest

CSRC = Path(__file__).resolve().parent.parent / "naturaldiffusion_amd" / "csrc"
LISTINGS = [CSRC / "build" / f"{unit}-hip-amdgcn-amd-amdhsa-gfx950.s" for unit in ("ncsnpp", "stream_guard")]

# (unguarded instance, guarded instance) as substrings of the mangled names
DMA = ["k_gemm_dmaILi2ELi2ELi4ELi4ELi2ELi%dEE", "k_gemm_ringILi2ELi2ELi8ELi4ELi3ELi%dEE", "k_gemm_ringILi2ELi2ELi2ELi4ELi4ELi%dEE", "k_gemm_dmaILi2ELi4ELi8ELi4ELi6ELi%dEE",
       "k_gemm_w128ILi%dEN"]
FP8 = ["k_gemm_fp8ILb0ELi%dEE", "k_gemm_fp8ILb1ELi%dEE", "k_gemm_w128_fp8ILb0ELi%dEE", "k_gemm_w128_fp8ILb1ELi%dEE"]
PAIRS = [(t % 7, t % 10) for t in DMA] + [(t % 3, t % 4) for t in FP8] + \
        [("k_splitk_reduce_f32ILb0EE", "k_splitk_reduce_f32ILb1EE"), ("k_patch_embedILb1ELb0EE", "k_patch_embedILb1ELb1EE"), ("k_patch_embedILb0ELb0EE", "k_patch_embedILb0ELb1EE")]


@pytest.fixture(scope="module")
def listing():
    subprocess.check_call(["make", "-C", str(CSRC), "-j4"], stdout=subprocess.DEVNULL)       # no-op when up to date
    bodies, meta = {}, {}
    for path in LISTINGS:
        text = path.read_text()
        for m in re.finditer(r"^(_Z\w+):\s*(?:;[^\n]*)?\n(.*?)^\.Lfunc_end\d+:", text, re.M | re.S):
            bodies[m.group(1)] = m.group(2)
        md = text[text.index("amdhsa.kernels:"):]
        for blk in re.split(r"\n  - \.", md)[1:]:
            name = re.search(r"\.name:\s*(\S+)", blk).group(1)
            get = lambda key: int(re.search(r"\." + key + r":\s*(\S+)", blk).group(1))
            meta[name] = dict(vgpr=get("vgpr_count"), vspill=get("vgpr_spill_count"), sspill=get("sgpr_spill_count"), scratch=get("private_segment_fixed_size"),
                              unit=path.name.split("-")[0])
    return bodies, meta


def _one(meta, sub, unit):
    hit = [n for n in meta if sub in n and meta[n]["unit"] == unit]
    assert len(hit) == 1, (sub, hit)
    return hit[0]


def _ops(body):
    return Counter(m.group(1) for m in re.finditer(r"^\s+([a-z][a-z0-9_]+)\b", body, re.M))


@pytest.mark.parametrize("plain,guarded", PAIRS, ids=[g for _, g in PAIRS])
def test_guarded_instance(listing, plain, guarded):
    bodies, meta = listing
    p, g = _one(meta, plain, "ncsnpp"), _one(meta, guarded, "stream_guard")
    assert p in bodies and g in bodies
    ops_p, ops_g = _ops(bodies[p]), _ops(bodies[g])
    # the report: vector atomics on global memory, at least one unsigned max and one add
    assert ops_g["global_atomic_umax"] >= 1, {k: v for k, v in ops_g.items() if "atomic" in k}
    assert all(k.startswith("global_atomic_") for k in ops_g if "atomic" in k), [k for k in ops_g if "atomic" in k]
    if guarded != "k_patch_embedILb0ELb1EE":                  # (that instance writes an fp32 stream only: tracked, never clamped or counted)
        assert ops_g["global_atomic_add"] >= 1, {k: v for k, v in ops_g.items() if "atomic" in k}
        assert ops_g["v_med3_f32"] >= 1, "the clamp"
    # the same stores, nothing more: the guard changes what is stored, not how
    stores = lambda ops: {k: v for k, v in ops.items() if k.startswith("global_store") or k.startswith("buffer_store")}
    assert stores(ops_g) == stores(ops_p), (stores(ops_p), stores(ops_g))
    assert ops_g["v_mfma_f32_16x16x32_bf16"] == ops_p["v_mfma_f32_16x16x32_bf16"]
    # registers: no spill, no scratch, and the unguarded twin's step of the occupancy table (one, two or four waves per SIMD: 512 / 256 / 128 registers per lane)
    assert (meta[g]["vspill"], meta[g]["sspill"], meta[g]["scratch"]) == (0, 0, 0), meta[g]
    assert (meta[p]["vspill"], meta[p]["sspill"], meta[p]["scratch"]) == (0, 0, 0), meta[p]
    step = lambda v: 128 if v <= 128 else 256 if v <= 256 else 512
    assert step(meta[g]["vgpr"]) <= step(meta[p]["vgpr"]), (meta[p], meta[g])
    # the unguarded twin reports nothing
    assert not any("atomic" in k for k in ops_p), [k for k in ops_p if "atomic" in k]
