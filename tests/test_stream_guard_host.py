"""The stream guard of the transformer engines on the host (no GPU): the C ABI of NATINF_DIT_STREAM_GUARD / NATINF_MMDIT_STREAM_GUARD (flags, site count, workspace
size, the status entries' refusals) and the fallback logic of ``generate_sharded(stream16="auto")`` against fake denoisers -- a guarded half-stream stand-in whose
status says "clamped" in chosen batches, and an fp32-stream stand-in that computes something recognisably different."""
import ctypes as C

import numpy as np
import pytest
import torch

EINVAL = -1
NEW_SYMBOLS = [f"natinf_{e}_stream_{f}" for e in ("dit", "mmdit") for f in ("sites", "status_reset", "status")]


def _dit(depth, hidden, heads, size, flags):
    from naturaldiffusion_amd._lib import lib
    h = C.c_void_p()
    rc = lib.natinf_dit_create_sized(C.byref(h), depth, hidden, heads, size, flags)
    return rc, h


def test_new_symbols_are_exported_and_declared(repo_root):
    from naturaldiffusion_amd import _lib
    text = {e: (repo_root / "include" / f"natinf_{e}.h").read_text() for e in ("dit", "mmdit")}
    for n in NEW_SYMBOLS:
        assert hasattr(_lib.lib, n) and n in _lib.SIGNATURES, n
        assert n + "(" in text[n.split("_")[1]], f"{n} is not declared in its header"
    assert "#define NATINF_DIT_STREAM_GUARD 16" in text["dit"] and "#define NATINF_MMDIT_STREAM_GUARD 2" in text["mmdit"]
    assert _lib.DIT_STREAM_GUARD == 16 and _lib.MMDIT_STREAM_GUARD == 2


@pytest.mark.parametrize("size", [32, 64])
@pytest.mark.parametrize("other", [0, 1, 2, 3], ids=["plain", "unfused", "fp8", "fp8_unfused"])
@pytest.mark.parametrize("s16", [0, 1])
def test_dit_guard_flag_sites_and_workspace(size, other, s16):
    from naturaldiffusion_amd._lib import lib, DIT_STREAM_GUARD
    depth = 3
    assert lib.natinf_set_dit_stream16(s16) == 0
    try:
        rc, plain = _dit(depth, 256, 4, size, other)
        assert rc == 0
        rc, g = _dit(depth, 256, 4, size, other | DIT_STREAM_GUARD)
        assert rc == 0, "the guard flag must combine with fp8, unfused attention, both input sizes and both stream formats"
    finally:
        lib.natinf_set_dit_stream16(-1)
    try:
        sites = lib.natinf_dit_stream_sites(g)
        assert sites == 1 + 2 * depth
        assert lib.natinf_dit_stream_sites(plain) < 0                               # an unguarded handle has no status block
        for mb in (1, 5, 16):
            assert lib.natinf_dit_workspace_bytes(g, mb) >= lib.natinf_dit_workspace_bytes(plain, mb) + 8 * sites
        # the guard adds a block, not a buffer per image
        assert lib.natinf_dit_workspace_bytes(g, 16) - lib.natinf_dit_workspace_bytes(plain, 16) == \
            lib.natinf_dit_workspace_bytes(g, 1) - lib.natinf_dit_workspace_bytes(plain, 1)
        assert lib.natinf_dit_param_count(g) == lib.natinf_dit_param_count(plain)
        assert lib.natinf_dit_packed_bytes(g) == lib.natinf_dit_packed_bytes(plain)
        # refusals that need no device: no workspace, no output, an unguarded handle
        assert lib.natinf_dit_stream_status_reset(g, None, None) == EINVAL
        assert lib.natinf_dit_stream_status(g, None, None, None) == EINVAL
        assert lib.natinf_dit_stream_status_reset(plain, C.c_void_p(256), None) == EINVAL
        assert lib.natinf_dit_stream_status(plain, C.c_void_p(256), C.c_void_p(256), None) == EINVAL
        assert lib.natinf_dit_stream_sites(None) < 0
    finally:
        lib.natinf_dit_destroy(g)
        lib.natinf_dit_destroy(plain)


def test_stray_flag_bits_are_still_invalid():
    from naturaldiffusion_amd._lib import lib, DIT_STREAM_GUARD, MMDIT_STREAM_GUARD
    rc, h = _dit(2, 128, 2, 32, DIT_STREAM_GUARD)                                   # the guard bit alone is a flag ...
    assert rc == 0 and h
    lib.natinf_dit_destroy(h)
    h = C.c_void_p()
    assert lib.natinf_mmdit_create(C.byref(h), 2, 2, 64, 32, 16, 8, 13, MMDIT_STREAM_GUARD) == 0 and h
    lib.natinf_mmdit_destroy(h)
    for flags in (4, 8, 6, 7, 16 | 8, 16 | 4, 32, 7 | 64, 1 << 20, 1 << 30):
        rc, h = _dit(2, 128, 2, 32, flags)
        assert rc == EINVAL and not h, flags
    h = C.c_void_p()
    for flags in (4, 8, 2 | 4, 1 << 20):
        assert lib.natinf_mmdit_create(C.byref(h), 2, 2, 64, 32, 16, 8, 13, flags) == EINVAL and not h, flags
    rc, h = _dit(2, 192, 2, 32, 2 | 16)                                             # fp8 still needs hidden % 128 == 0, guarded or not
    assert rc == EINVAL


@pytest.mark.parametrize("fp8", [0, 1])
def test_mmdit_guard_flag_sites_and_workspace(fp8):
    from naturaldiffusion_amd._lib import lib, MMDIT_STREAM_GUARD
    layers = 3
    hs = []
    for flags in (fp8, fp8 | MMDIT_STREAM_GUARD):
        h = C.c_void_p()
        assert lib.natinf_mmdit_create(C.byref(h), layers, 2, 64, 32, 16, 8, 13, flags) == 0
        hs.append(h)
    plain, g = hs
    try:
        sites = lib.natinf_mmdit_stream_sites(g)
        assert sites == 1 + 2 * layers and lib.natinf_mmdit_stream_sites(plain) < 0
        for mb in (1, 4):
            assert lib.natinf_mmdit_workspace_bytes(g, mb) >= lib.natinf_mmdit_workspace_bytes(plain, mb) + 8 * sites
        assert lib.natinf_mmdit_stream_status_reset(plain, C.c_void_p(256), None) == EINVAL
        assert lib.natinf_mmdit_stream_status(g, None, None, None) == EINVAL
    finally:
        lib.natinf_mmdit_destroy(g)
        lib.natinf_mmdit_destroy(plain)


# ------------------------------------------------------------------------------ the job's fallback logic
class FakeSampler:
    """ValidateNI's place in generate_sharded: z' = 0.5 z - 0.1 (uncond + cfg (cond - uncond)) + 0.01 noise, the first 4 of 8 channels (CPU tensors)"""

    def __init__(self, C_, B, node, c1, c2, E, device=None, seed=0, elems_per_image=None):
        self.per = elems_per_image

    def step(self, kk, z, cond, uncond, cfg, per, stride, noise=None, index=None):
        n = z.numel() // per
        c, u = cond.reshape(n, stride)[:, :per], uncond.reshape(n, stride)[:, :per]
        return (0.5 * z.reshape(n, per) - 0.1 * (u + cfg * (c - u)) + 0.01 * noise.reshape(n, per)).reshape(-1)


def fake_noise(indices, shape, seed, device, column=0):
    return torch.stack([torch.randn(shape, generator=torch.Generator().manual_seed(1000 * seed + i)) for i in indices])


class FakeEngine:
    """forward = a smooth function of (z, t, y) scaled by ``gain`` (the half and the fp32 stand-ins differ in it, so a batch says which one made it).  Guarded:
    the status after a batch (= since the last reset) says "clamped" when that batch's position is in ``clamp_batches``."""
    input_size = 32
    max_batch = 64
    site_names = ["patch_embed", "blocks.0.attn", "blocks.0.mlp", "blocks.1.attn", "blocks.1.mlp"]

    def __init__(self, gain, guard=False, clamp_batches=()):
        self.gain, self.guard, self.clamp_batches = gain, guard, set(clamp_batches)
        self.resets = self.reads = self.forwards = 0

    def forward(self, z, t, y):
        self.forwards += 1
        w = (y.float() / 1000.0 + t.float() / 999.0)[:, None, None, None]
        return torch.cat([self.gain * torch.tanh(z) * w, z * 0], dim=1)

    def reset_stream_status(self):
        assert self.guard
        self.resets += 1

    def stream_status(self):
        assert self.guard
        self.reads += 1
        clamped = np.zeros(5, np.uint32)
        max_abs = np.array([3.0, 5.0, 9.0, 11.0, 40.0], np.float32)
        if self.resets - 1 in self.clamp_batches:
            clamped[3:] = (7, 2)
            max_abs[3:] = (1.5e5, 2.5e5)
        return {"max_abs": max_abs, "clamped": clamped}


@pytest.fixture
def cpu_job(monkeypatch):
    from naturaldiffusion_amd import ValidateNaturalInference as V
    from naturaldiffusion_amd import CIFAR10NaturalInference as Cf
    monkeypatch.setattr(V, "ValidateNI", FakeSampler)
    monkeypatch.setattr(Cf, "philox_noise", fake_noise)
    monkeypatch.setattr(V, "device", "cpu")
    monkeypatch.setattr(V, "denoiser_factory", None)
    monkeypatch.setattr(V, "model_path", None)
    return V


def test_auto_reruns_exactly_the_clamped_batch(cpu_job):
    V = cpu_job
    kw = dict(alg_name="ddim", num_step=18, batch_size=3, seed=3, decode=False)
    half_ref = V.generate_sharded(10, None, model=FakeEngine(1.0), **kw)[0]           # four batches: 3 + 3 + 3 + 1
    wide_ref = V.generate_sharded(10, None, model=FakeEngine(1.25), **kw)[0]
    assert not torch.equal(half_ref[3:6], wide_ref[3:6])
    half, wide, made, report = FakeEngine(1.0, guard=True, clamp_batches=[1]), FakeEngine(1.25), [], {}

    def fallback():
        made.append(1)
        return wide
    z, lab, idx, img = V.generate_sharded(10, None, model=half, stream16="auto", fallback=fallback, report=report, **kw)
    assert torch.equal(z[3:6], wide_ref[3:6]), "the clamped batch must be the fp32-stream engine's"
    assert torch.equal(z[:3], half_ref[:3]) and torch.equal(z[6:], half_ref[6:]), "the other batches must be untouched"
    assert idx.tolist() == list(range(10)) and img is None
    assert report["rerun_batches"] == [1] and report["batches"] == 4
    assert report["first_clamp"] == dict(batch=1, site=3, site_name="blocks.1.attn", max_abs=1.5e5, clamped=7)
    assert len(made) == 1 and wide.forwards == 18, "the fp32-stream engine is built once and runs that one batch"
    assert half.resets == 4 and half.reads == 4 and half.forwards == 4 * 18          # reset in front of every batch, ONE read behind it


def test_auto_without_a_clamp_never_builds_the_fallback(cpu_job):
    V = cpu_job
    kw = dict(alg_name="ddim", num_step=18, batch_size=4, seed=1, decode=False)
    ref = V.generate_sharded(8, None, model=FakeEngine(1.0), **kw)[0]
    report = {}

    def fallback():
        raise AssertionError("no batch clamped: the fp32-stream engine must not be built")
    z = V.generate_sharded(8, None, model=FakeEngine(1.0, guard=True), stream16="auto", fallback=fallback, report=report, **kw)[0]
    assert torch.equal(z, ref) and report == dict(batches=2, rerun_batches=[], first_clamp=None)
    # every batch clamps: every batch reruns, the engine is still built once
    wide, made, report = FakeEngine(1.25), [], {}
    z = V.generate_sharded(8, None, model=FakeEngine(1.0, guard=True, clamp_batches=[0, 1]), stream16="auto",
                           fallback=lambda: (made.append(1), wide)[1], report=report, **kw)[0]
    assert torch.equal(z, V.generate_sharded(8, None, model=FakeEngine(1.25), **kw)[0])
    assert report["rerun_batches"] == [0, 1] and report["first_clamp"]["batch"] == 0 and len(made) == 1


@pytest.mark.parametrize("mode", [None, True, False])
def test_other_modes_never_touch_a_guard(cpu_job, mode):
    V = cpu_job
    kw = dict(alg_name="ddim", num_step=18, batch_size=4, seed=1, decode=False)

    class Unguarded(FakeEngine):
        def reset_stream_status(self):
            raise AssertionError("status reset outside auto mode")

        def stream_status(self):
            raise AssertionError("status read outside auto mode")
    ref = V.generate_sharded(8, None, model=FakeEngine(1.0), **kw)[0]
    rep = {}
    assert torch.equal(V.generate_sharded(8, None, model=Unguarded(1.0), stream16=mode, report=rep, **kw)[0], ref)
    assert rep == dict(batches=2, rerun_batches=[], first_clamp=None)
    # ... and the engine the job builds from model_path is asked for in that very mode: never "auto", never guarded
    asked = []

    def loader(path, max_batch=16, fp8=False, stream16=None):
        asked.append((path, max_batch, fp8, stream16))
        return Unguarded(1.0)
    V.model_path = "weights.pt"
    V.load_dit_engine, keep = loader, V.load_dit_engine
    try:
        assert torch.equal(V.generate_sharded(8, None, stream16=mode, **kw)[0], ref)
    finally:
        V.load_dit_engine = keep
    assert asked == [("weights.pt", 8, False, mode)]


def test_auto_builds_both_engines_from_model_path_lazily(cpu_job):
    V = cpu_job
    kw = dict(alg_name="ddim", num_step=18, batch_size=4, seed=1, decode=False)
    asked = []

    def loader(path, max_batch=16, fp8=False, stream16=None):
        asked.append(stream16)
        return FakeEngine(1.0, guard=True, clamp_batches=[1]) if stream16 == "auto" else FakeEngine(1.25)
    V.model_path = "weights.pt"
    V.load_dit_engine, keep = loader, V.load_dit_engine
    try:
        rep = {}
        V.generate_sharded(4, None, stream16="auto", report=rep, **kw)            # one batch, in range
        assert asked == ["auto"] and rep["rerun_batches"] == []
        V.generate_sharded(8, None, stream16="auto", report=rep, **kw)            # the second batch clamps
        assert asked == ["auto", "auto", False] and rep["rerun_batches"] == [1]
    finally:
        V.load_dit_engine = keep


def test_auto_refusals(cpu_job):
    V = cpu_job
    kw = dict(alg_name="ddim", num_step=18, batch_size=4, decode=False)
    with pytest.raises(ValueError, match="guarded"):
        V.generate_sharded(4, None, model=FakeEngine(1.0), stream16="auto", fallback=lambda: FakeEngine(1.0), **kw)
    with pytest.raises(ValueError, match="fallback"):
        V.generate_sharded(4, None, model=FakeEngine(1.0, guard=True), stream16="auto", **kw)
    with pytest.raises(ValueError, match="stream16"):
        V.generate_sharded(4, None, model=FakeEngine(1.0), stream16="half", **kw)
    with pytest.raises(ValueError, match="stream16"):
        V.load_dit_engine("nowhere.pt", stream16="half")


def test_site_names_follow_the_status_block():
    from naturaldiffusion_amd._lib import StreamGuardStatus, lib, DIT_STREAM_GUARD
    rc, h = _dit(2, 128, 2, 32, DIT_STREAM_GUARD)
    assert rc == 0

    class Probe(StreamGuardStatus):
        _guard_api = "natinf_dit"
    p = Probe()
    p._h, p.guard = h, True
    try:
        assert p.site_names == ["patch_embed", "blocks.0.attn", "blocks.0.mlp", "blocks.1.attn", "blocks.1.mlp"]
        p.guard = False
        with pytest.raises(RuntimeError):
            p.site_names
    finally:
        lib.natinf_dit_destroy(h)
