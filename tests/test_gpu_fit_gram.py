"""natinf_fit_gram_f64 on the GPU (include/natinf_fit.h): against the longdouble oracle within the bound any summation order meets, exactly on small
integers, bitwise symmetric, the same bytes for any split of the images over calls, and nothing read or written outside what the header names."""
import ctypes

import numpy as np
import pytest
import torch

import fit_oracle as O
from naturaldiffusion_amd import _lib
from naturaldiffusion_amd import fit as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _slots(n_rows):
    """non-contiguous, strictly ascending: 0, 2, 5, 7, 10, ..."""
    return [(5 * t + 1) // 2 for t in range(n_rows)]


def _problem(n_img, epi, n_rows, seed, integers=False, pad_images=1):
    """A history slab of more slots and a longer row than the call uses, NaN wherever the call must not read; noise and target.  -> host arrays and
    the per-image stacks [n_img, M, epi] (fp64 values of what the kernel reads)"""
    rng = np.random.default_rng(seed)
    slots = _slots(n_rows)
    n_slot, stride = slots[-1] + 3, (n_img + pad_images) * epi
    hist = np.full((n_slot, stride), np.nan)
    if integers:
        draw = lambda shape: rng.integers(-8, 9, shape).astype(np.float64)
        rows = draw((n_rows, n_img * epi))
        noise, target = draw(n_img * epi).astype(np.float32), draw(n_img * epi).astype(np.float32)
    else:
        scale = lambda n: 10.0 ** rng.uniform(-3, 3, (n, 1))
        rows = rng.standard_normal((n_rows, n_img * epi)) * scale(n_rows)
        noise = (rng.standard_normal(n_img * epi) * scale(1)[0]).astype(np.float32)
        target = (rng.standard_normal(n_img * epi) * scale(1)[0]).astype(np.float32)
    hist[slots, :n_img * epi] = rows
    stacks = np.stack([np.vstack([rows[:, i * epi:(i + 1) * epi], noise[None, i * epi:(i + 1) * epi].astype(np.float64),
                                  target[None, i * epi:(i + 1) * epi].astype(np.float64)]) for i in range(n_img)])
    dev = lambda a: torch.from_numpy(a).to(DEV)
    return dict(slots=slots, hist=dev(hist), noise=dev(noise), target=dev(target), stacks=stacks, n_img=n_img, epi=epi)


def _gram(p, n_images=None, first=0):
    return F.gram(p["hist"], p["slots"], p["noise"], p["target"], p["n_img"] if n_images is None else n_images, p["epi"], first_image=first)


@pytest.mark.parametrize("n_rows", [1, 5, 14, 15, 30])
@pytest.mark.parametrize("epi", [4, 1028, 3072])
def test_gram_against_longdouble_oracle(epi, n_rows):
    """M = 3, 7, 16, 17, 32: both sides of the 16-wide tile edge and the maximum.  |G - oracle| <= gamma_E sum_e |v_a v_b|, the bound of ANY order of
    summation: a miss is wrong arithmetic, not an unlucky order.  The unread history slots hold NaN, so a finite result read none of them."""
    p = _problem(3, epi, n_rows, seed=100 * n_rows + epi)
    G = _gram(p)
    assert G.shape == (3, n_rows + 2, n_rows + 2) and G.dtype == torch.float64
    got = G.cpu().numpy()
    assert np.isfinite(got).all()
    assert torch.equal(G, G.transpose(1, 2))                                   # bitwise: NaN-free, so equal values are equal bytes up to the sign of 0
    assert np.array_equal(got.view(np.uint64), got.transpose(0, 2, 1).copy().view(np.uint64))
    worst = 0.0
    for i in range(3):
        want, mag = O.gram(p["stacks"][i], rounded=False)
        err = np.abs(got[i].astype(np.longdouble) - want)
        bound = O.gamma(epi) * mag
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), (i, float((err / bound).max()))
    print(f"fit gram epi={epi} M={n_rows + 2}: worst error / bound = {worst:.3g}")


@pytest.mark.parametrize("n_rows,epi", [(5, 1028), (15, 1028), (30, 3072)])
def test_gram_is_exact_on_small_integers(n_rows, epi):
    p = _problem(3, epi, n_rows, seed=7, integers=True)
    want = np.stack([s.astype(np.int64) @ s.astype(np.int64).T for s in p["stacks"]])
    got = _gram(p).cpu().numpy()
    assert np.array_equal(got, want.astype(np.float64))


@pytest.mark.parametrize("n_rows", [5, 15])
def test_split_of_the_images_gives_the_same_bytes(n_rows):
    p = _problem(5, 1028, n_rows, seed=21)
    whole = _gram(p)
    two = torch.cat([_gram(p, 2, 0), _gram(p, 3, 2)])
    alone = torch.cat([_gram(p, 1, i) for i in range(5)])
    as_bits = lambda t: t.cpu().numpy().view(np.uint64)
    assert np.array_equal(as_bits(whole), as_bits(two)) and np.array_equal(as_bits(whole), as_bits(alone))


@pytest.mark.parametrize("n_rows", [5, 15])
def test_nothing_past_the_output_is_written(n_rows):
    p = _problem(3, 1028, n_rows, seed=33)
    M = n_rows + 2
    sentinel = -1234.5
    out = torch.full((3 * M * M + 64,), sentinel, dtype=torch.float64, device=DEV)
    rows_c = (ctypes.c_int32 * n_rows)(*p["slots"])
    _lib.check(_lib.lib.natinf_fit_gram_f64(_lib.ptr(p["hist"]), int(p["hist"].shape[1]), rows_c, n_rows, _lib.ptr(p["noise"]), _lib.ptr(p["target"]),
                                            3, 1028, _lib.ptr(out), _lib.stream_ptr()), "natinf_fit_gram_f64")
    assert (out[3 * M * M:] == sentinel).all()
    assert torch.equal(out[:3 * M * M].view(3, M, M), _gram(p))
