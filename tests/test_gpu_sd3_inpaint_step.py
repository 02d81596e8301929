"""GPU tests of the SD3-form inpainting step (natinf_step_f16chain_inpaint) and of the blend on its own (natinf_known_blend_f16), include/natinf.h.
Two yardsticks, neither of them the fused kernel: the existing per-image entry natinf_step_f16chain_guided followed by the blend entry, and a NumPy
fp16 restatement written here the way ``oracle.ni_oracle``'s SD3 step is written -- every product, sum and quotient formed in fp32 from fp16 operands
and rounded to fp16, scalars fp32.  The fresh noise of the restatement is natinf_randn_philox_col_f32's, rounded to fp16 once.  Each case computes
its references once and shares them."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

K = 3                                                          # history rows of the synthetic matrix
W = np.array([[0.75, 0.0, 0.0], [0.3, 0.625, 0.0], [0.21, 0.33, 0.41]])
SIG = torch.tensor([0.9, 0.71, 0.52, 0.3], dtype=torch.float32)
H = lambda t: float(t.to(torch.float16))                       # 0-d fp32 tensor -> the fp16 value eager PyTorch multiplies by
SEED = 0x1234567887654321
COL0 = 2 ** 31
BLEND_MEAN = 2
SHAPES = [(8, 3), (4096, 5), (2056, 3)]                        # one vector per image; the job's test latent; 771 vectors: no multiple of the 256-thread block
F16, F32 = np.float16, np.float32


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from naturaldiffusion_amd import _lib
    _lib.require_gpu()
    return torch.device("cuda:0")


# ---- the NumPy restatement: fp32 math on fp16 operands, one rounding to fp16 per operation ----
def hmul(s, a):
    return (F32(s) * a.astype(F32)).astype(F16)


def hadd(a, b):
    return (a.astype(F32) + b.astype(F32)).astype(F16)


def hsub(a, b):
    return (a.astype(F32) - b.astype(F32)).astype(F16)


def flow(n, m, sig, oms):
    return hadd(hmul(sig, n), hmul(oms, m))


class Case:
    """n images of ``se`` elements; slots [-1, 0, 1, -1, 2, ...], distinct scales; random fp16 x, v_text, v_null, noise, known, a K-row history and a
    byte mask with whole 8-vectors of zeros, whole vectors of non-zeros and mixed ones (CPU copies kept)"""

    def __init__(self, dev, se, n, seed):
        from naturaldiffusion_amd.coeff import SparseRows
        gen = torch.Generator().manual_seed(seed)
        rnd = lambda *s: torch.randn(*s, generator=gen).half()
        self.dev, self.n, self.se, self.E = dev, n, se, n * se
        self.slots, g = [], 0
        for i in range(n):
            self.slots.append(-1 if i % 3 == 0 else g)
            g += i % 3 != 0
        self.g = g
        self.scales = [1.3 + 0.7 * i for i in range(n)]
        self.x, self.vt, self.noise, self.known = rnd(self.E), rnd(self.E), rnd(self.E), rnd(self.E) * 1.7
        self.vn, self.hist0 = rnd(g * se), rnd(K, self.E) * 1.3
        bits = torch.randint(0, 2, (self.E,), generator=gen, dtype=torch.uint8) * torch.randint(1, 256, (self.E,), generator=gen, dtype=torch.int32).to(torch.uint8)
        kind = (torch.randperm(self.E // 8, generator=gen) % 3).repeat_interleave(8)         # per 8-vector, a third each -- 0: no known element, 1: all known, 2: mixed
        self.mask = torch.where(kind == 0, torch.zeros_like(bits), torch.where(kind == 1, bits.clamp(min=1), bits)).contiguous()
        self.index = [7 + 5 * i * i for i in range(n)]                                        # no arithmetic progression
        self.d = {name: getattr(self, name).to(dev) for name in ("x", "vt", "noise", "vn", "known", "mask")}
        self.d["index"] = torch.tensor(self.index, dtype=torch.int64, device=dev)
        self.d["cfg"] = torch.tensor(self.scales, dtype=torch.float32, device=dev)
        self.d["slot"] = torch.tensor(self.slots, dtype=torch.int32, device=dev)
        self.rows = SparseRows(W, lambda k: k + 1, torch.float32, dev, dense=True)
        self._fresh, self._guided = {}, {}

    def fresh(self, column, index=None):
        """the fresh noise of a column: natinf_randn_philox_col_f32 for the case's global indices, rounded to fp16 once -> CPU [E]"""
        from naturaldiffusion_amd.CIFAR10NaturalInference import philox_noise
        key = (column, tuple(index or self.index))
        if key not in self._fresh:
            self._fresh[key] = philox_noise(list(key[1]), (self.se,), SEED, self.dev, column=column).half().reshape(-1).cpu()
        return self._fresh[key]

    def _outs(self, k):
        hist = self.hist0.to(self.dev)
        hist[k:] = 0
        return hist, torch.zeros(self.E, dtype=torch.float16, device=self.dev), torch.zeros(self.E, dtype=torch.float16, device=self.dev)

    def _head(self, k, hist, mean, xn, velocity, ov):
        from naturaldiffusion_amd._lib import ptr
        idx, val, nt = self.rows.ptrs(k)
        r = self.rows.rows[k]
        d = self.d
        return (ptr(d["x"]), ptr(d["vt"]), ptr(d["vn"]) if ov.get("vn", True) else None, ptr(d["cfg"]),
                ptr(ov.get("slot", d["slot"])), ov.get("n_uncond", self.g), ov.get("se", self.se),
                ptr(d["noise"]) if ov.get("noise", True) else None, ptr(hist), ptr(mean) if ov.get("want_mean", True) else None,
                ptr(xn) if ov.get("want_next", True) else None, idx, val, nt, r.diag, r.total, k, H(SIG[k]), H(SIG[k + 1]), H(1 - SIG[k + 1]),
                ov.get("flags", 1 if velocity else 0), ov.get("E", self.E))

    def guided(self, k, velocity):
        """natinf_step_f16chain_guided, once per (k, velocity) -> (hist, mean, x_next) on the CPU"""
        from naturaldiffusion_amd._lib import lib, stream_ptr
        if (k, velocity) not in self._guided:
            hist, mean, xn = self._outs(k)
            assert lib.natinf_step_f16chain_guided(*self._head(k, hist, mean, xn, velocity, {}), stream_ptr()) == 0
            torch.cuda.synchronize()
            self._guided[(k, velocity)] = (hist.cpu(), mean.cpu(), xn.cpu())
        return self._guided[(k, velocity)]

    def tail(self, column, form, ov):
        """the trailing arguments of the step: known, mask, strides, column, seed, index arguments"""
        from naturaldiffusion_amd._lib import ptr
        known, mask = ov.get("known_t", self.d["known"]), ov.get("mask_t", self.d["mask"])
        index = (ptr(self.d["index"]), 0, 0) if form == "array" else (None, 100, 3)
        return (ptr(known) if ov.get("known", True) else None, ptr(mask) if ov.get("mask", True) else None,
                ov.get("ks", self.se if known.numel() == self.E and self.n > 1 else 0), ov.get("ms", self.se if mask.numel() == self.E and self.n > 1 else 0),
                column, SEED, *index)

    def blend(self, x_in, k, column, form="array", **ov):
        """natinf_known_blend_f16 at level k + 1 on a CPU tensor -> (rc, out on the CPU; zero-filled before the call)"""
        from naturaldiffusion_amd._lib import lib, ptr, stream_ptr
        xin, out = x_in.to(self.dev), torch.zeros(self.E, dtype=torch.float16, device=self.dev)
        t = self.tail(column, form, ov)
        rc = lib.natinf_known_blend_f16(ptr(xin), ptr(out), ptr(self.d["noise"]) if ov.get("noise", True) else None, t[0], t[1], t[2], t[3],
                                        H(SIG[k + 1]), H(1 - SIG[k + 1]), t[4], t[5], t[6], t[7], t[8], ov.get("se", self.se), ov.get("E", self.E), stream_ptr())
        torch.cuda.synchronize()
        return rc, out.cpu()

    def inpaint(self, k, velocity, column, form="array", **ov):
        """natinf_step_f16chain_inpaint -> (rc, hist, mean, x_next) on the CPU, the three outputs zero-filled before the call"""
        from naturaldiffusion_amd._lib import lib, stream_ptr
        hist, mean, xn = self._outs(k)
        rc = lib.natinf_step_f16chain_inpaint(*self._head(k, hist, mean, xn, velocity, ov), *self.tail(column, form, ov), stream_ptr())
        torch.cuda.synchronize()
        return rc, hist.cpu(), mean.cpu(), xn.cpu()

    def restated(self, k, velocity, nz):
        """the NumPy restatement of the fused step -> (hist[k], mean, x_next, blended mean) as fp16 arrays; ``nz`` the noise side [E] fp16"""
        sig, sn, on = F32(H(SIG[k])), F32(H(SIG[k + 1])), F32(H(1 - SIG[k + 1]))
        x, vt = self.x.numpy().reshape(self.n, self.se), self.vt.numpy().reshape(self.n, self.se)
        vn = self.vn.numpy().reshape(self.g, self.se)
        f = np.empty_like(x)
        for i, (slot, cfg) in enumerate(zip(self.slots, self.scales)):
            if slot < 0:
                f[i] = hsub(x[i], hmul(sig, vt[i]))
            elif velocity:
                v = hadd(vn[slot], hmul(cfg, hsub(vt[i], vn[slot])))
                f[i] = hsub(x[i], hmul(sig, v))
            else:
                x0n, x0t = hsub(x[i], hmul(sig, vn[slot])), hsub(x[i], hmul(sig, vt[i]))
                f[i] = hadd(x0n, hmul(cfg, hsub(x0t, x0n)))
        f = f.reshape(-1)
        acc, tot = np.zeros(self.E, F16), 0.0
        for j in range(k + 1):
            acc = hadd(acc, hmul(W[k][j], self.hist0[j].numpy() if j < k else f))
            tot = tot + W[k][j]
        mean = (acc.astype(F32) / F32(tot)).astype(F16)
        m, known = self.mask.numpy() != 0, self.known.numpy()
        x_next = np.where(m, flow(nz.numpy(), known, sn, on), flow(self.noise.numpy(), mean, sn, on))
        return f, mean, x_next, np.where(m, known, mean)


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: "%dx%d" % s)
def case(dev, request):
    se, n = request.param
    return Case(dev, se, n, seed=11 + se)


def same_bytes(a, b):
    a = a.numpy() if isinstance(a, torch.Tensor) else a
    b = b.numpy() if isinstance(b, torch.Tensor) else b
    return a.shape == b.shape and np.array_equal(a.view(np.uint16), b.view(np.uint16))


@pytest.mark.parametrize("renoise", ["fresh", "same"])
@pytest.mark.parametrize("velocity", [False, True])
@pytest.mark.parametrize("k", [0, 2])
def test_fused_step_is_guided_step_then_blend_and_the_restatement(case, k, velocity, renoise):
    column = COL0 + k + 1 if renoise == "fresh" else 0
    hist_g, mean_g, xn_g = case.guided(k, velocity)
    rc_b, want = case.blend(xn_g, k, column)
    rc, hist, mean, xn = case.inpaint(k, velocity, column)
    assert rc == 0 and rc_b == 0
    m = case.mask != 0
    assert bool(m.any()) and bool((~m).any()) and torch.isfinite(want.float()).all()
    assert not torch.equal(want, xn_g)                                     # the blend does something
    assert same_bytes(xn, want), "x_next is not the guided step followed by the blend"
    assert same_bytes(hist, hist_g), "the history saw the blend"
    assert same_bytes(mean, mean_g), "mean_out without the flag is not the guided entry's"
    # the NumPy restatement, on the same parameters
    f, r_mean, r_next, _ = case.restated(k, velocity, case.fresh(column) if column else case.noise)
    assert same_bytes(hist[k], f) and same_bytes(mean, r_mean) and same_bytes(xn, r_next)


def test_first_index_and_stride_form(case):
    """image i has global index 100 + 3*i: the bytes of the index array [100, 103, ...]"""
    k, column = 2, COL0 + 3
    rc, _, _, xn = case.inpaint(k, False, column, form="stride")
    f, _, r_next, _ = case.restated(k, False, case.fresh(column, [100 + 3 * i for i in range(case.n)]))
    assert rc == 0 and same_bytes(xn, r_next)
    rc_b, want = case.blend(case.guided(k, False)[2], k, column, form="stride")
    assert rc_b == 0 and same_bytes(xn, want)
    assert not same_bytes(xn, case.inpaint(k, False, column)[3])           # and the index does reach the draw


def test_all_zero_mask_is_the_guided_entry(case):
    zero = torch.zeros(case.E, dtype=torch.uint8, device=case.dev)
    for column in (0, COL0 + 1):
        rc, hist, mean, xn = case.inpaint(0, False, column, mask_t=zero, flags=BLEND_MEAN)
        hist_g, mean_g, xn_g = case.guided(0, False)
        assert rc == 0 and same_bytes(hist, hist_g) and same_bytes(mean, mean_g) and same_bytes(xn, xn_g)


def test_all_one_mask_keeps_a_nan_of_the_unknown_side_out(case):
    ones = torch.ones(case.E, dtype=torch.uint8, device=case.dev)
    vt = case.d["vt"].clone()
    case.d["vt"][::5] = float("nan")
    try:
        rc, hist, mean, xn = case.inpaint(2, False, COL0 + 3, mask_t=ones, flags=BLEND_MEAN)
    finally:
        case.d["vt"].copy_(vt)
    assert rc == 0 and torch.isnan(hist[2].float()).any()                  # the NaN is in the history, as the guided entry leaves it
    sn, on = np.float32(H(SIG[3])), np.float32(H(1 - SIG[3]))
    assert torch.isfinite(xn.float()).all() and same_bytes(xn, flow(case.fresh(COL0 + 3).numpy(), case.known.numpy(), sn, on))
    assert same_bytes(mean, case.known)                                    # and the blended mean is `known` itself


@pytest.mark.parametrize("velocity", [False, True])
def test_blend_mean_flag(case, velocity):
    """NATINF_SD3_BLEND_MEAN: mean_out = where(mask, known, mean); x_next and hist[k] as without it; x_next NULL (the job's last step) as well"""
    k, column = 2, COL0 + 3
    hist_g, mean_g, _ = case.guided(k, velocity)
    want = torch.where(case.mask != 0, case.known, mean_g)
    _, _, _, r_bmean = case.restated(k, velocity, case.fresh(column))
    assert same_bytes(want, r_bmean)
    base = case.inpaint(k, velocity, column)
    rc, hist, mean, xn = case.inpaint(k, velocity, column, flags=BLEND_MEAN | (1 if velocity else 0))
    assert rc == 0 and same_bytes(mean, want) and same_bytes(xn, base[3]) and same_bytes(hist, hist_g)
    for column in (COL0 + 3, 0):                                           # "same" mode without x_next needs no noise either
        rc, hist, mean, xn = case.inpaint(k, velocity, column, flags=BLEND_MEAN | (1 if velocity else 0), want_next=False, noise=column != 0)
        assert rc == 0 and same_bytes(mean, want) and same_bytes(hist, hist_g) and not bool(xn.any())


def test_shared_rows_are_the_expanded_rows(case):
    """a stride of 0: one row of known / mask for every image == that row repeated"""
    k, column, se = 2, COL0 + 3, case.se
    known1, mask1 = case.known[:se].contiguous().to(case.dev), case.mask[:se].contiguous().to(case.dev)
    rc_a, _, mean_a, xn_a = case.inpaint(k, False, column, known_t=known1, mask_t=mask1, ks=0, ms=0, flags=BLEND_MEAN)
    rc_b, _, mean_b, xn_b = case.inpaint(k, False, column, known_t=known1.repeat(case.n), mask_t=mask1.repeat(case.n), ks=se, ms=se, flags=BLEND_MEAN)
    assert rc_a == 0 and rc_b == 0 and same_bytes(xn_a, xn_b) and same_bytes(mean_a, mean_b)
    assert not same_bytes(xn_a, case.inpaint(k, False, column)[3])
    # one of the two shared, and the blend entry takes the same strides
    rc_c, _, _, xn_c = case.inpaint(k, False, column, mask_t=mask1, ms=0)
    rc_d, want = case.blend(case.guided(k, False)[2], k, column, mask_t=mask1, ms=0)
    assert rc_c == 0 and rc_d == 0 and same_bytes(xn_c, want)


@pytest.mark.parametrize("euler", [False, True])
def test_uniform_scale_and_slots_give_the_launch_wide_bytes_on_the_unknown_side(dev, repo_root, euler):
    """through ``SD3NI``: cfg_image = full(cfg), uncond_slot = arange(n) -> natinf_step_f16chain's hist[k] and mean, and its x_next where the mask is 0;
    the first input is natinf_flow_input_f16's where the mask is 0"""
    from oracle import ni_oracle as O
    from naturaldiffusion_amd.sampler import SD3NI
    weights = None if euler else O.load_sd3_csv(repo_root / "weights/sd3_step_28_weight.csv")
    _, sigmas = O.sd3_sigma_schedule(28)
    for se, n in SHAPES:
        E, k = n * se, 2
        gen = torch.Generator().manual_seed(se)
        x, vt, vn, nz, known = [torch.randn(E, generator=gen).half().to(dev) for _ in range(5)]
        mask = (torch.rand(E, generator=gen) < 0.5).to(torch.uint8).to(dev)
        hist = (torch.randn(k, E, generator=gen) * 1.3).half().to(dev)
        a, b = SD3NI(weights, sigmas, E, device=dev, cfg=3.7, euler=euler), SD3NI(weights, sigmas, E, device=dev, euler=euler, elems_per_image=se)
        a.hist[:k], b.hist[:k] = hist, hist
        mean_a, next_a = a.step(k, x, vt, vn, nz)
        kw = dict(cfg=torch.full((n,), 3.7, device=dev), uncond_slot=torch.arange(n, dtype=torch.int32, device=dev))
        for renoise in ("fresh", "same"):
            mean_b, next_b = b.step(k, x, vt, vn, nz, known=known, mask=mask, seed=SEED, index=(4, 2), renoise=renoise, **kw)
            assert torch.equal(a.hist[k], b.hist[k]) and torch.equal(mean_a, mean_b)
            assert torch.equal(torch.where(mask != 0, next_a, next_b), next_a) and not torch.equal(next_a, next_b)
            mean_c, none = b.step(k, x, vt, vn, nz, want_next=False, known=known, mask=mask, seed=SEED, index=(4, 2), renoise=renoise, blend_mean=True, **kw)
            assert none is None and torch.equal(mean_c, torch.where(mask != 0, known, mean_a))
            x0_a = a.first_input(nz).clone()
            x0_b = b.first_input(nz, known, mask, seed=SEED, index=(4, 2), renoise=renoise)
            assert torch.equal(torch.where(mask != 0, x0_a, x0_b), x0_a) and torch.isfinite(x0_b.float()).all()
            # level 0 is pure noise (sigma_0 = 1): "same" gives the image's own noise back, "fresh" another draw on the known elements
            assert torch.equal(x0_a, x0_b) == (renoise == "same")


def test_refusals_leave_zero_filled_outputs_untouched(dev):
    """every refusal is NATINF_EINVAL and launches nothing: the guided entry's, the blend's, and the blend entry's own"""
    case = Case(dev, 24, 5, seed=3)
    column = COL0 + 3
    odd = torch.zeros(case.E + 8, dtype=torch.uint8, device=dev)[4:4 + case.E]             # a mask 4 bytes off an 8-byte boundary
    assert odd.data_ptr() % 8 == 4
    bad_slot = lambda v: torch.tensor([-1, 0, v, -1, 2], dtype=torch.int32, device=dev)
    step = [dict(slot=bad_slot(3)), dict(slot=bad_slot(-2)), dict(se=12), dict(se=16), dict(vn=False), dict(flags=4), dict(flags=7), dict(n_uncond=-1),
            dict(E=case.E + 4), dict(noise=False),                                             # the guided entry's
            dict(known=False), dict(mask=False), dict(ks=8), dict(ms=case.E), dict(ks=-case.se), dict(mask_t=odd)]   # the blend's
    for ov in step:
        rc, hist, mean, xn = case.inpaint(2, False, column, **ov)
        assert rc == -1, ov
        assert torch.equal(hist[:2], case.hist0[:2]) and not bool(hist[2:].any()) and not bool(mean.any()) and not bool(xn.any()), ov
    for col in (1, 29, COL0 - 1):                                                              # a column that is neither "same" nor "fresh"
        rc, hist, mean, xn = case.inpaint(2, False, col)
        assert rc == -1 and not bool(hist[2:].any()) and not bool(mean.any()) and not bool(xn.any()), col
    for col, ov in ((column, dict(known=False)), (column, dict(mask=False)), (column, dict(ks=8)), (column, dict(ms=16)), (column, dict(mask_t=odd)),
                    (column, dict(se=12)), (column, dict(se=16)), (column, dict(E=case.E + 4)), (1, {}), (COL0 - 1, {}), (0, dict(noise=False))):
        rc, out = case.blend(case.x, 2, col, **ov)
        assert rc == -1 and not bool(out.any()), (col, ov)
    assert case.inpaint(2, False, column)[0] == 0 and case.inpaint(2, False, 0)[0] == 0       # and the good calls go through
    assert case.blend(case.x, 2, column, noise=False)[0] == 0                                  # "fresh" reads no noise


def test_sampler_refusals(dev, repo_root):
    """``SD3NI``'s own checks are host-side ``ValueError``s made before any launch"""
    from oracle import ni_oracle as O
    from naturaldiffusion_amd.sampler import SD3NI
    Wt = O.load_sd3_csv(repo_root / "weights/sd3_step_28_weight.csv")
    _, sigmas = O.sd3_sigma_schedule(28)
    n, se = 5, 24
    E = n * se
    ni = SD3NI(Wt, sigmas, E, device=dev, elems_per_image=se)
    gen = torch.Generator().manual_seed(5)
    x, vt, vn, nz, known = [torch.randn(E, generator=gen).half().to(dev) for _ in range(5)]
    mask = torch.ones(E, dtype=torch.uint8, device=dev)
    kw = dict(cfg=torch.full((n,), 4.0, device=dev), uncond_slot=torch.arange(n, dtype=torch.int32, device=dev))
    before = ni.hist.clone()
    bad = [dict(known=known, mask=None), dict(known=None, mask=mask), dict(known=known.float(), mask=mask), dict(known=known, mask=mask.bool()),
           dict(known=known[:40], mask=mask), dict(known=known, mask=mask.cpu()), dict(known=known, mask=mask, renoise="other"),
           dict(known=known, mask=mask, seed=None), dict(known=known, mask=torch.ones(E + 8, dtype=torch.uint8, device=dev)[4:4 + E])]
    for b in bad:
        b = {"seed": 1, **b}
        with pytest.raises(ValueError):
            ni.step(0, x, vt, vn, nz, **kw, **b)
        with pytest.raises(ValueError):
            ni.first_input(nz, b.pop("known"), b.pop("mask"), **b)
    with pytest.raises(ValueError):                                                    # the launch-wide form has no blend
        ni.step(0, x, vt, vn, nz, known=known, mask=mask, seed=1)
    with pytest.raises(ValueError):                                                    # blend_mean without known / mask
        ni.step(0, x, vt, vn, nz, blend_mean=True, **kw)
    torch.cuda.synchronize()
    assert torch.equal(ni.hist.view(torch.int16), before.view(torch.int16)), "a refused call launched"
    mean, xn = ni.step(0, x, vt, vn, nz, known=known, mask=mask, renoise="same", **kw)  # "same" needs no seed
    torch.cuda.synchronize()
    assert torch.isfinite(xn.float()).all()
