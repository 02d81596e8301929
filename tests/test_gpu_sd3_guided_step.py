"""GPU tests of the SD3-form step with per-image guidance (natinf_step_f16chain_guided, include/natinf.h), through the C entry and through
``sampler.SD3NI.step(cfg=<tensor>, uncond_slot=...)``.  Two yardsticks, neither of them the new kernel: the existing entry
natinf_step_f16chain (the identity rule) and a CPU restatement in eager torch fp16 -- ``oracle.ni_oracle.sd3_weighted_mean`` plus the
per-image expressions of the header, written the way ``test_sd3_full_size_step_matches_oracle`` writes them (0-d fp32 tensors for the
sigmas, Python floats for the scales and weights: eager PyTorch's own casts)."""
import numpy as np
import pytest
import torch

from oracle import ni_oracle as O

pytestmark = pytest.mark.gpu

K = 3                                                          # history rows of the synthetic matrix
W = np.array([[0.75, 0.0, 0.0], [0.3, 0.625, 0.0], [0.21, 0.33, 0.41]])
SIG = torch.tensor([0.9, 0.71, 0.52, 0.3], dtype=torch.float32)
H = lambda t: float(t.to(torch.float16))                       # 0-d fp32 tensor -> the fp16 value eager PyTorch multiplies by


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from naturaldiffusion_amd import _lib
    _lib.require_gpu()
    return torch.device("cuda:0")


class Case:
    """n images of ``se`` elements, g null-prompt rows; random fp16 x, v_text, v_null, noise and a K-row history (CPU copies kept)"""

    def __init__(self, dev, n, se, g, seed):
        from naturaldiffusion_amd.coeff import SparseRows
        gen = torch.Generator().manual_seed(seed)
        rnd = lambda *s: torch.randn(*s, generator=gen).half()
        self.dev, self.n, self.se, self.g, self.E = dev, n, se, g, n * se
        self.x, self.vt, self.noise, self.hist0 = rnd(n * se), rnd(n * se), rnd(n * se), rnd(K, n * se) * 1.3
        self.vn = rnd(max(g, 1) * se)[:g * se]
        self.d = {name: getattr(self, name).to(dev) for name in ("x", "vt", "noise", "vn")}
        self.rows = SparseRows(W, lambda k: k + 1, torch.float32, dev, dense=True)

    def launch(self, k, slots, scales, velocity, *, n_uncond=None, vn="own", want_mean=True, want_next=True, se=None, flags=None, E=None):
        """natinf_step_f16chain_guided -> (rc, hist, mean, x_next) with the three outputs pre-filled with 9.0"""
        from naturaldiffusion_amd._lib import lib, ptr, stream_ptr
        hist = self.hist0.to(self.dev)
        hist[k:] = 9.0
        mean, xn = torch.full((self.E,), 9.0, dtype=torch.float16, device=self.dev), torch.full((self.E,), 9.0, dtype=torch.float16, device=self.dev)
        cfg_t = torch.tensor(scales, dtype=torch.float32, device=self.dev)
        slot_t = torch.tensor(slots, dtype=torch.int32, device=self.dev)
        vn_t = (self.d["vn"] if self.g else None) if isinstance(vn, str) else vn
        idx, val, nt = self.rows.ptrs(k)
        r = self.rows.rows[k]
        rc = lib.natinf_step_f16chain_guided(ptr(self.d["x"]), ptr(self.d["vt"]), ptr(vn_t), ptr(cfg_t), ptr(slot_t),
                                             self.g if n_uncond is None else n_uncond, self.se if se is None else se,
                                             ptr(self.d["noise"]), ptr(hist), ptr(mean) if want_mean else None, ptr(xn) if want_next else None,
                                             idx, val, nt, r.diag, r.total, k, H(SIG[k]), H(SIG[k + 1]), H(1 - SIG[k + 1]),
                                             (1 if velocity else 0) if flags is None else flags, self.E if E is None else E, stream_ptr())
        torch.cuda.synchronize()
        return rc, hist.cpu(), mean.cpu(), xn.cpu()

    def restated(self, k, slots, scales, velocity):
        """the CPU restatement -> (hist[k], mean, x_next)"""
        sig, sn = SIG[k], SIG[k + 1]
        x, vt, vn = self.x.view(self.n, self.se), self.vt.view(self.n, self.se), self.vn.view(self.g, self.se)
        f = torch.empty_like(x)
        for i, (slot, cfg) in enumerate(zip(slots, scales)):
            if slot < 0:
                f[i] = x[i] - sig * vt[i]
            elif velocity:
                v = vn[slot] + float(cfg) * (vt[i] - vn[slot])
                f[i] = x[i] - sig * v
            else:
                x0n = x[i] - sig * vn[slot]
                x0t = x[i] - sig * vt[i]
                f[i] = x0n + float(cfg) * (x0t - x0n)
        f = f.reshape(-1)
        mean = O.sd3_weighted_mean([self.hist0[j] for j in range(k)] + [f], W[:k + 1, :k + 1])
        return f, mean, sn * self.noise + (1 - sn) * mean

    def check(self, k, slots, scales, velocity):
        rc, hist, mean, xn = self.launch(k, slots, scales, velocity)
        assert rc == 0
        f, want_mean, want_next = self.restated(k, slots, scales, velocity)
        assert torch.isfinite(want_next.float()).all() and float(want_next.float().abs().max()) > 0
        tag = (k, slots, scales, velocity)
        assert np.array_equal(hist[k].numpy().view(np.uint16), f.numpy().view(np.uint16)), ("hist[k]", tag)
        assert np.array_equal(mean.numpy().view(np.uint16), want_mean.numpy().view(np.uint16)), ("mean", tag)
        assert np.array_equal(xn.numpy().view(np.uint16), want_next.numpy().view(np.uint16)), ("x_next", tag)
        assert torch.equal(hist[:k], self.hist0[:k]) and bool((hist[k + 1:] == 9.0).all()), "the step wrote a history row other than k"


@pytest.fixture(scope="module")
def small(dev):
    return Case(dev, n=5, se=24, g=3, seed=1)                   # three 8-vectors per image: image boundaries fall inside a wave


@pytest.fixture(scope="module")
def stride(dev):
    return Case(dev, n=17, se=16 * 128 * 128, g=9, seed=2)      # 557,056 vectors > kMaxGrid * kBlock = 524,288: the loop's second trip


@pytest.mark.parametrize("euler", [False, True])
@pytest.mark.parametrize("k", [0, 2])
def test_identity_rule(dev, repo_root, euler, k):
    """uncond_slot = arange(n) and cfg_image = full(cfg): hist[k], mean and x_next are the bytes of natinf_step_f16chain, through ``SD3NI.step`` both ways"""
    from naturaldiffusion_amd.sampler import SD3NI
    weights = None if euler else O.load_sd3_csv(repo_root / "weights/sd3_step_28_weight.csv")
    _, sigmas = O.sd3_sigma_schedule(28)
    for n, se, seed in ((5, 24, 3), (3, 4096, 4)):
        E = n * se
        gen = torch.Generator().manual_seed(seed)
        x, vt, vn, nz = [torch.randn(E, generator=gen).half().to(dev) for _ in range(4)]
        hist = (torch.randn(k, E, generator=gen) * 1.3).half().to(dev)
        a, b = SD3NI(weights, sigmas, E, device=dev, cfg=3.7, euler=euler), SD3NI(weights, sigmas, E, device=dev, euler=euler, elems_per_image=se)
        a.hist[:k], b.hist[:k] = hist, hist
        mean_a, next_a = a.step(k, x, vt, vn, nz)
        mean_b, next_b = b.step(k, x, vt, vn, nz, cfg=torch.full((n,), 3.7, device=dev), uncond_slot=torch.arange(n, dtype=torch.int32, device=dev))
        assert torch.isfinite(next_a.float()).all() and float(next_a.float().abs().max()) > 0
        assert torch.equal(a.hist[k], b.hist[k]) and torch.equal(mean_a, mean_b) and torch.equal(next_a, next_b)
        assert torch.equal(b.hist[:k], hist)
        # sample_elems given per call is the same launch; the last step wants no x_next
        c = SD3NI(weights, sigmas, E, device=dev, euler=euler)
        c.hist[:k] = hist
        mean_c, next_c = c.step(k, x, vt, vn, nz, want_next=False, cfg=torch.full((n,), 3.7, device=dev),
                                uncond_slot=torch.arange(n, dtype=torch.int32, device=dev), n_uncond=n, sample_elems=se)
        assert next_c is None and torch.equal(mean_c, mean_a) and torch.equal(c.hist[k], a.hist[k])


@pytest.mark.parametrize("velocity", [False, True])
@pytest.mark.parametrize("k", [0, 2])
def test_mixed_launch_smallest_shape(small, k, velocity):
    """5 images of 24 elements, 3 null-prompt rows, distinct scales (1.3 is no fp16 or fp32 number), the scales on a slot of -1 ignored"""
    small.check(k, [-1, 0, -1, 1, 2], [4.0, 7.0, 2.5, 1.3, 3.5], velocity)


@pytest.mark.parametrize("velocity", [False, True])
def test_mixed_launch_over_the_grid_stride_boundary(stride, velocity):
    """17 images of 16 x 128 x 128 elements, 3-row history: E / 8 exceeds the 524,288 vectors one trip of the grid-stride loop covers"""
    assert stride.E // 8 > 2048 * 256
    slots = [0, -1, 1, 2, -1, 3, -1, 4, 5, -1, -1, 6, 7, -1, -1, -1, 8]         # the last image, in the second trip, is guided
    stride.check(2, slots, [1.5 + 0.25 * i for i in range(17)], velocity)


@pytest.mark.parametrize("velocity", [False, True])
def test_shared_rows_and_pointer_variants(dev, small, velocity):
    # one row of v_null serves two images, scales repeat, a row is left out
    small.check(2, [1, 1, -1, 0, 0], [4.0, 2.5, 3.0, 4.0, 4.0], velocity)
    slots, scales = [-1, 0, -1, 1, 2], [4.0, 7.0, 2.5, 1.3, 3.5]
    f, want_mean, want_next = small.restated(2, slots, scales, velocity)
    # x_next None: mean and hist[k] written, x_next untouched; mean_out None likewise
    rc, hist, mean, xn = small.launch(2, slots, scales, velocity, want_next=False)
    assert rc == 0 and torch.equal(hist[2], f) and torch.equal(mean, want_mean) and bool((xn == 9.0).all())
    rc, hist, mean, xn = small.launch(2, slots, scales, velocity, want_mean=False)
    assert rc == 0 and torch.equal(hist[2], f) and torch.equal(xn, want_next) and bool((mean == 9.0).all())
    # v_null NULL with every slot -1 (n_uncond = 0): f = x - sig*v_text for both flags
    none = Case(dev, n=5, se=24, g=0, seed=1)
    none.check(2, [-1] * 5, [7.0] * 5, velocity)
    rc, hist, _, _ = none.launch(0, [-1] * 5, [7.0] * 5, velocity)
    assert rc == 0 and torch.equal(hist[0], none.x - SIG[0] * none.vt)
    # every slot -1 with rows present: the rows are not read into anything
    rc, hist, mean, xn = small.launch(2, [-1] * 5, scales, velocity)
    assert rc == 0 and torch.equal(hist[2], small.x - SIG[2] * small.vt)


def test_refusals_launch_nothing(small):
    """each refusal is NATINF_EINVAL and leaves hist, mean and x_next as they were"""
    ok_slots, scales = [-1, 0, -1, 1, 2], [4.0, 7.0, 2.5, 1.3, 3.5]
    refusals = [dict(slots=[-1, 0, 3, 1, 2]),                                   # a slot equal to n_uncond
                dict(slots=[-1, 0, -2, 1, 2]),                                  # a slot of -2
                dict(slots=[2 ** 31 - 1, 0, 0, 0, 0]),
                dict(se=12),                                                    # not a multiple of 8
                dict(se=16),                                                    # does not divide E = 120
                dict(vn=None),                                                  # n_uncond = 3 with NULL v_null
                dict(flags=2), dict(flags=3),                                   # an unknown flag bit
                dict(n_uncond=-1), dict(E=124)]
    for kw in refusals:
        kw = dict(kw)
        rc, hist, mean, xn = small.launch(2, kw.pop("slots", ok_slots), scales, False, **kw)
        assert rc == -1, kw
        assert torch.equal(hist[:2], small.hist0[:2]) and bool((hist[2:] == 9.0).all()) and bool((mean == 9.0).all()) and bool((xn == 9.0).all()), kw
    assert small.launch(2, ok_slots, scales, False)[0] == 0


def test_sampler_refusals(dev, repo_root):
    """``SD3NI``'s own checks are host-side ``ValueError``s; a bad slot surfaces as the entry's "invalid argument" """
    from naturaldiffusion_amd.sampler import SD3NI
    Wt = O.load_sd3_csv(repo_root / "weights/sd3_step_28_weight.csv")
    _, sigmas = O.sd3_sigma_schedule(28)
    n, se = 5, 24
    E = n * se
    for bad in (12, 16, 0, -8, 7):
        with pytest.raises(ValueError):
            SD3NI(Wt, sigmas, E, device=dev, elems_per_image=bad)
    ni = SD3NI(Wt, sigmas, E, device=dev, elems_per_image=se)
    gen = torch.Generator().manual_seed(5)
    x, vt, nz = [torch.randn(E, generator=gen).half().to(dev) for _ in range(3)]
    vn = torch.randn(3 * se, generator=gen).half().to(dev)
    cfg = torch.full((n,), 4.0, device=dev)
    ok = torch.tensor([0, 1, 2, -1, -1], dtype=torch.int32, device=dev)
    before = ni.hist.clone()
    for args in ((cfg.double(), ok), (cfg.cpu(), ok), (cfg[:4], ok), (cfg, ok.long()), (cfg, ok.cpu()), (cfg, ok[:4]), (cfg, None)):
        with pytest.raises(ValueError):
            ni.step(0, x, vt, vn, nz, cfg=args[0], uncond_slot=args[1])
    with pytest.raises(ValueError):                                                    # slots without per-image scales
        ni.step(0, x, vt, vn, nz, uncond_slot=ok)
    with pytest.raises(ValueError):                                                    # a float scale belongs to the constructor
        ni.step(0, x, vt, vn, nz, cfg=4.0)
    with pytest.raises(ValueError):                                                    # not the pinned per-image size
        ni.step(0, x, vt, vn, nz, cfg=cfg, uncond_slot=ok, sample_elems=40)
    with pytest.raises(ValueError):                                                    # no per-image size at all
        SD3NI(Wt, sigmas, E, device=dev).step(0, x, vt, vn, nz, cfg=cfg, uncond_slot=ok)
    for bad in ([0, 1, 3, -1, -1], [0, -2, 1, 2, -1]):
        with pytest.raises(RuntimeError, match="invalid argument"):
            ni.step(0, x, vt, vn, nz, cfg=cfg, uncond_slot=torch.tensor(bad, dtype=torch.int32, device=dev))
    with pytest.raises(RuntimeError, match="invalid argument"):                       # a slot 0 with no row at all
        ni.step(0, x, vt, None, nz, cfg=cfg, uncond_slot=torch.zeros(n, dtype=torch.int32, device=dev))
    torch.cuda.synchronize()
    assert torch.equal(ni.hist.view(torch.int16), before.view(torch.int16)), "a refused call launched"
    mean, xn = ni.step(0, x, vt, vn, nz, cfg=cfg, uncond_slot=ok)                      # and the good call goes through
    torch.cuda.synchronize()
    assert torch.isfinite(xn.float()).all()
