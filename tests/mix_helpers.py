"""Host restatement (numpy only) of hwgat_mix_draw, hwgat_mix_apply and the pair loss of hwgat_mbsce_fwd, written from the
comment of include/hwgat_hip.h ("Mixup and temporal CutMix of the pairs of a batch").  `mix32` is the restated dropout hash
of tests/mask_helpers.py, `perm` / `uniform` the loader's restated permutation and tagged uniform of
tests/loader_helpers.py.  Nothing here calls into the library.

Whatever a floating-point value decides is checked to lie more than MARGIN from its boundary -- Joehnk's X + Y against 1,
u against prob / cutmix_share, the two floor arguments against an integer -- and the assertion says "choose another seed":
a difference between a device integer and this file is then a bug and not an ulp of a libm's pow.  tests/test_mix_cpu.py
checks that the (seed, step, B, n) of the GPU tests trip none of them."""
import numpy as np

from loader_helpers import perm, uniform
from mask_helpers import mix32

MIX_TAG, TAG_APPLY, TAG_MODE, TAG_BETA, TAG_START = 2, 0x10, 0x20, 0x30, 0x40
NONE, MIXUP, CUTMIX = 0, 1, 2
ALPHA_MIN, BETA_TRIES = 0.05, 64
MARGIN = 1e-9

# what tests/test_gpu_mix.py draws (and tests/test_mix_cpu.py checks against the margins)
DRAW_SEED, DRAW_STEP0, DRAW_STEPS, DRAW_T = 20, 5, 3, 16
DRAW_SHAPES = [(1, 1), (2, 2), (7, 7), (8, 5), (8, 0), (64, 63)]
DRAW_PROBS = [0.0, 1.0, 0.5]
DRAW_SHARES = [0.0, 1.0, 0.5]
DRAW_ALPHAS = (0.4, 1.0)           # (mixup_alpha, cutmix_alpha)


def _far(v, edge, what):
    assert abs(v - edge) > MARGIN, f"{what} = {v!r} lies within {MARGIN} of {edge!r}: choose another seed"


def _far_from_integer(v, what):
    _far(v, np.round(v), what)


def step_keys(seed, step):
    """(K_step, K_sigma) of one draw"""
    k_step = int(mix32(seed, (MIX_TAG << 32) + int(step)))
    return k_step, int(mix32(k_step, 0))


def pair_key(k_step, p):
    return int(mix32(k_step, 1 + int(p)))


def matching(seed, step, n):
    """(pairs (n // 2, 2), the unpaired live row or None)"""
    _, k_sigma = step_keys(seed, step)
    sigma = perm(k_sigma, n, np.arange(n)) if n > 0 else np.zeros(0, dtype=np.int64)
    return sigma[:2 * (n // 2)].reshape(-1, 2), (int(sigma[n - 1]) if n % 2 else None)


def johnk(key, alpha, check=True):
    """lambda0 ~ Beta(alpha, alpha) from the uniforms of `key`: (value, tries used)"""
    inv = np.float64(1.0) / np.float64(alpha)
    for k in range(BETA_TRIES):
        X = np.power(np.float64(uniform(key, TAG_BETA, 2 * k)), inv)
        Y = np.power(np.float64(uniform(key, TAG_BETA, 2 * k + 1)), inv)
        S = X + Y
        if check:
            _far(S, 1.0, "X + Y")
        if 0.0 < S <= 1.0:
            return X / S, k + 1
    return np.float64(0.5), BETA_TRIES


def draw(seed, step, y, n, T, prob=1.0, cutmix_share=0.5, mixup_alpha=0.4, cutmix_alpha=1.0):
    """one hwgat_mix_draw on the targets y (B,) with n live rows: dict(pairs, partner, lam, seg, mode, y_b)"""
    y = np.asarray(y, dtype=np.int64)
    B = len(y)
    assert 0 <= n <= B and ALPHA_MIN <= mixup_alpha <= 1.0 and ALPHA_MIN <= cutmix_alpha <= 1.0
    k_step, _ = step_keys(seed, step)
    found, _ = matching(seed, step, n)
    pairs = np.full((max(B // 2, 1), 2), -1, dtype=np.int32)
    pairs[:n // 2] = found
    partner = np.arange(B, dtype=np.int32)
    lam = np.ones(B, dtype=np.float32)
    seg = np.zeros((B, 2), dtype=np.int32)
    mode = np.zeros(B, dtype=np.int32)
    for p, (a, b) in enumerate(found):
        key = pair_key(k_step, p)
        u = float(uniform(key, TAG_APPLY, 0))
        if 0.0 < prob < 1.0:
            _far(u, prob, "u_apply")
        if not u < prob:
            continue
        u = float(uniform(key, TAG_MODE, 0))
        if 0.0 < cutmix_share < 1.0:
            _far(u, cutmix_share, "u_mode")
        cut = u < cutmix_share
        l0, _ = johnk(key, cutmix_alpha if cut else mixup_alpha)
        if cut:
            v = (np.float64(1.0) - l0) * np.float64(T) + 0.5
            _far_from_integer(v, "(1 - lambda0) T + 0.5")
            L = int(min(max(np.floor(v), 0), T))
            v = np.float64(uniform(key, TAG_START, 0)) * np.float64(T - L + 1)
            _far_from_integer(v, "u_start (T - L + 1)")
            t0 = int(min(np.floor(v), T - L))
            lam[[a, b]] = np.float32(np.float64(T - L) / np.float64(T))
            seg[[a, b]] = (t0, L)
            mode[[a, b]] = CUTMIX
        else:
            lam[[a, b]] = np.float32(l0)
            mode[[a, b]] = MIXUP
        partner[a], partner[b] = b, a
    return dict(pairs=pairs, partner=partner, lam=lam, seg=seg, mode=mode, y_b=y[partner])


def apply(x, rec, n):
    """hwgat_mix_apply on x (B, T, ...) float32 with the records of a draw (the helper's or the device's): a new array"""
    x = np.asarray(x)
    assert x.dtype == np.float32
    out = x.copy()
    for a, b in np.asarray(rec["pairs"])[:n // 2]:
        md = int(rec["mode"][a])
        if md == MIXUP:
            l = np.float32(rec["lam"][a])
            w = np.float32(np.float32(1.0) - l)
            out[a] = (l * x[a]).astype(np.float32) + (w * x[b]).astype(np.float32)       # each product and the sum in fp32
            out[b] = (l * x[b]).astype(np.float32) + (w * x[a]).astype(np.float32)
        elif md == CUTMIX:
            t0, L = (int(v) for v in rec["seg"][a])
            out[a, t0:t0 + L] = x[b, t0:t0 + L]
            out[b, t0:t0 + L] = x[a, t0:t0 + L]
    return out


def row_losses(z, y, eps):
    """l(y) per row in z's precision: (1 - eps)(lse - z_y) + eps (lse - mean z)"""
    z = np.asarray(z)
    m = z.max(-1, keepdims=True)
    lse = (m + np.log(np.exp(z - m).sum(-1, keepdims=True)))[:, 0]
    return (1.0 - eps) * (lse - z[np.arange(len(y)), y]) + eps * (lse - z.mean(-1))


def pair_losses(z, y, y_b, lam, eps):
    """lam l(y) + (1 - lam) l(y_b) per row"""
    lam = np.asarray(lam).astype(z.dtype)
    return lam * row_losses(z, y, eps) + (1.0 - lam) * row_losses(z, y_b, eps)


def dominant(y, y_b, lam):
    return np.where(np.asarray(lam) >= np.float32(0.5), y, y_b)
