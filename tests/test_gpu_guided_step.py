"""GPU tests of the Validate-form step with per-image guidance (natinf_step_f32prod_noise_guided, include/natinf.h) through
``sampler.ValidateNI.step(cfg=<tensor>, uncond_slot=...)``.  The yardstick is the existing entry natinf_step_f32prod_noise, never
the new one: a step is a per-image function, so the expected bytes of a mixed launch are the existing entry run once per
group of images that share a scale (``uncond=None`` for the images without a slot), each sub-launch on those images'
``image_index`` and on their columns of the ``hist_x0`` rows."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SEED = 40211
N = 6                                                          # steps of the synthetic matrix


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from naturaldiffusion_amd import _lib
    _lib.require_gpu()
    return torch.device("cuda:0")


def matrices():
    """a 6-step matrix: C lower triangular and dense (row 5: five history terms and the diagonal); B row 0 = columns 0 and 1
    (the step at k = 0: no history, the initial noise plus the first draw), row 5 = columns 0, 3 and 6"""
    r = np.random.RandomState(5)
    C = np.tril(r.uniform(0.1, 0.9, (N, N)))
    B = np.zeros((N, N + 1))
    B[0, :2] = (0.7, 0.3)
    for k in range(1, N):
        B[k, 0] = 0.2 + 0.1 * k
    B[5, 3], B[5, 6] = 0.45, 0.35
    node = np.stack([np.linspace(900, 100, N + 1), np.ones(N + 1), np.zeros(N + 1)], 1)
    c1 = np.linspace(3.0, 1.01, N).astype(np.float32)
    c2 = np.linspace(2.8, 0.15, N).astype(np.float32)
    return C, B, node, c1, c2


class Case:
    """n images of ``se`` elements; cond [n, st] and uncond [g, st] hold a sample's eps in their first ``se`` columns (``make_eps`` may
    give them the [., 8, S, S] shape of a DiT output); random z, history, noise; non-contiguous global indices"""

    def __init__(self, dev, n, se, st, g, seed, shape=None):
        gen = torch.Generator().manual_seed(seed)
        rnd = lambda *s: torch.randn(*s, generator=gen).to(dev)
        self.n, self.se, self.st, self.g, self.E = n, se, st, g, n * se
        self.z, self.noise, self.hist0 = rnd(n * se), rnd(n * se), rnd(N, n * se)
        self.cond, self.uncond = rnd(n, st), rnd(max(g, 1), st)[:g]
        if shape is not None:
            self.cond, self.uncond = self.cond.view(n, *shape), self.uncond.view(g, *shape)
        self.idx = [(2 ** 33 + 5 if i == 1 else 977 * i + 3) for i in range(n)]
        self.index = torch.tensor(self.idx, dtype=torch.int64, device=dev)
        self.dev = dev

    def sampler(self, E):
        from naturaldiffusion_amd.sampler import ValidateNI
        C, B, node, c1, c2 = matrices()
        return ValidateNI(C, B, node, c1, c2, E, device=self.dev, seed=SEED, elems_per_image=self.se)

    def guided(self, k, slots, scales):
        """the entry under test -> (z_next, hist_x0 after the step)"""
        ni = self.sampler(self.E)
        ni.hist_x0.copy_(self.hist0)
        out = ni.step(k, self.z, self.cond, self.uncond if self.g else None, torch.tensor(scales, dtype=torch.float32, device=self.dev), self.se, self.st,
                      noise=self.noise, index=self.index, uncond_slot=torch.tensor(slots, dtype=torch.int32, device=self.dev), n_uncond=self.g)
        return out.clone(), ni.hist_x0.clone()

    def existing(self, k, images, cfg, rows):
        """natinf_step_f32prod_noise on the images ``images`` alone: one scale, ``rows`` their rows of uncond (None: uncond = NULL)"""
        m, sel = len(images), torch.tensor(images, device=self.dev)
        ni = self.sampler(m * self.se)
        ni.hist_x0.copy_(self.hist0.view(N, self.n, self.se)[:, sel].reshape(N, -1))
        cond = self.cond.reshape(self.n, self.st)[sel].contiguous()
        unc = None if rows is None else self.uncond.reshape(self.g, self.st)[torch.tensor(rows, device=self.dev)].contiguous()
        out = ni.step(k, self.z.view(self.n, self.se)[sel].reshape(-1).contiguous(), cond, unc, float(cfg), self.se, self.st,
                      noise=self.noise.view(self.n, self.se)[sel].reshape(-1).contiguous(), index=self.index[sel].contiguous())
        return out.view(m, self.se).clone(), ni.hist_x0.view(N, m, self.se).clone()

    def expected(self, k, slots, scales):
        """the per-group expectation -> (z_next, hist_x0 after the step)"""
        groups = {}
        for i, (s, c) in enumerate(zip(slots, scales)):
            groups.setdefault(None if s < 0 else float(np.float32(c)), []).append(i)
        z_next = torch.empty(self.n, self.se, device=self.dev)
        hist = self.hist0.clone().view(N, self.n, self.se)
        for cfg, images in groups.items():
            zs, hs = self.existing(k, images, 1.0 if cfg is None else cfg, None if cfg is None else [slots[i] for i in images])
            sel = torch.tensor(images, device=self.dev)
            z_next[sel] = zs
            hist[:, sel] = hs
        return z_next.reshape(-1), hist.reshape(N, -1)


def check(case, k, slots, scales):
    got_z, got_h = case.guided(k, slots, scales)
    want_z, want_h = case.expected(k, slots, scales)
    assert torch.isfinite(want_z).all() and float(want_z.abs().max()) > 0
    assert np.array_equal(got_z.cpu().numpy(), want_z.cpu().numpy()), ("z_next", k, slots, scales)
    assert np.array_equal(got_h[k].cpu().numpy(), want_h[k].cpu().numpy()), ("hist_x0[k]", k, slots, scales)
    keep = [j for j in range(N) if j != k]
    assert torch.equal(got_h[keep], case.hist0[keep]), "the step wrote a history row other than k"


@pytest.fixture(scope="module")
def small(dev):
    return Case(dev, n=5, se=8, st=16, g=3, seed=1)             # two quads per image: img = v / svec and q both matter


@pytest.fixture(scope="module")
def blocks(dev):
    return Case(dev, n=3, se=4 * 32 * 32, st=8 * 32 * 32, g=2, seed=2, shape=(8, 32, 32))     # 3,072 quads = 12 blocks


@pytest.mark.parametrize("k", [0, 5])
def test_identity_rule(dev, k):
    """uniform scale 4.0 with slots 0..n-1 is natinf_step_f32prod_noise(cfg = 4.0); every slot -1 is that entry with uncond = NULL"""
    for case in (Case(dev, n=5, se=8, st=16, g=5, seed=3), Case(dev, n=3, se=4096, st=8192, g=3, seed=4, shape=(8, 32, 32))):
        n = case.n
        got_z, got_h = case.guided(k, list(range(n)), [4.0] * n)
        want_z, want_h = case.existing(k, list(range(n)), 4.0, list(range(n)))
        assert np.array_equal(got_z.cpu().numpy(), want_z.reshape(-1).cpu().numpy())
        assert np.array_equal(got_h.cpu().numpy(), want_h.reshape(N, -1).cpu().numpy())
        got_z, got_h = case.guided(k, [-1] * n, [4.0] * n)
        want_z, want_h = case.existing(k, list(range(n)), 4.0, None)
        assert np.array_equal(got_z.cpu().numpy(), want_z.reshape(-1).cpu().numpy())
        assert np.array_equal(got_h.cpu().numpy(), want_h.reshape(N, -1).cpu().numpy())
    # no unconditional rows at all: uncond NULL, n_uncond 0
    none = Case(dev, n=5, se=8, st=16, g=0, seed=3)
    got_z, _ = none.guided(k, [-1] * 5, [4.0] * 5)
    assert np.array_equal(got_z.cpu().numpy(), none.existing(k, list(range(5)), 4.0, None)[0].reshape(-1).cpu().numpy())


@pytest.mark.parametrize("k", [0, 5])
def test_mixed_launch_smallest_shape(small, k):
    """5 images of 8 elements at stride 16, 3 unconditional rows, the slots a permutation, the 7 on a slot of -1 ignored"""
    check(small, k, [2, -1, 0, -1, 1], [4, 1, 2.5, 7, 1.5])


@pytest.mark.parametrize("k", [0, 5])
def test_mixed_launch_over_several_blocks(blocks, k):
    """3 images of 4 x 32 x 32 elements, the first 4 of 8 channels of [., 8, 32, 32] tensors"""
    check(blocks, k, [1, -1, 0], [4, 7, 2.5])


def test_a_row_may_serve_two_images_and_scales_may_repeat(small):
    check(small, 5, [1, 1, -1, 0, 2], [4, 2.5, 3, 4, 4])


def test_slot_refusals_launch_nothing(small):
    """a slot outside -1 .. n_uncond-1 is NATINF_EINVAL (read back before the launch), and so are the other refusals of the wrapper"""
    ni = small.sampler(small.E)
    ni.hist_x0.copy_(small.hist0)
    cfg = torch.full((5,), 4.0, device=small.dev)
    kw = dict(noise=small.noise, index=small.index)
    for bad in ([0, 1, 3, -1, -1], [0, -2, 1, 2, -1], [2 ** 31 - 1, 0, 0, 0, 0]):
        with pytest.raises(RuntimeError, match="invalid argument"):
            ni.step(5, small.z, small.cond, small.uncond, cfg, 8, 16, uncond_slot=torch.tensor(bad, dtype=torch.int32, device=small.dev), **kw)
    with pytest.raises(RuntimeError, match="invalid argument"):                       # a slot 0 with no row at all
        ni.step(5, small.z, small.cond, None, cfg, 8, 16, uncond_slot=torch.zeros(5, dtype=torch.int32, device=small.dev), **kw)
    torch.cuda.synchronize()
    assert torch.equal(ni.hist_x0, small.hist0), "a refused call launched"
    ok = torch.tensor([0, 1, 2, -1, -1], dtype=torch.int32, device=small.dev)
    for args in ((cfg.double(), ok), (cfg.cpu(), ok), (cfg[:4], ok), (cfg, ok.long()), (cfg, ok.cpu()), (cfg, ok[:4]), (cfg, None)):
        with pytest.raises(ValueError):
            ni.step(5, small.z, small.cond, small.uncond, args[0], 8, 16, uncond_slot=args[1], **kw)
    with pytest.raises(ValueError):                                                    # slots without per-image scales
        ni.step(5, small.z, small.cond, small.uncond, 4.0, 8, 16, uncond_slot=ok, **kw)
    with pytest.raises(ValueError):                                                    # per-image scales without noise= (the hist_eps-style call)
        ni.step(5, small.z, small.cond, small.uncond, cfg, 8, 16, uncond_slot=ok)
    from naturaldiffusion_amd.sampler import ValidateNI
    C, B, node, c1, c2 = matrices()
    slab = ValidateNI(C, B, node, c1, c2, small.E, device=small.dev)
    with pytest.raises(ValueError):                                                    # the slab form takes one float
        slab.step(5, small.z, small.cond, small.uncond, cfg, 8, 16, uncond_slot=ok)
    torch.cuda.synchronize()
