"""The host side of colour matching (MikuDanceVideoPipeline.__call__(color_match=...)): from the colour moments the device returns
(ops.color_moments: nine sums per frame) to the per-frame affine map the device applies (ops.color_apply: y = M s + t).  Float64 numpy,
3 x 3 systems, no torch: the UniPC precedent, small systems solved on the host.

    sums   s0, s1, s2, s0^2, s1^2, s2^2, s0 s1, s0 s2, s1 s2 summed over n pixels, s the displayed colour in [0, 1]
    mu     the channel means, sums[:3] / n
    Sigma  the 3 x 3 population covariance, E[s s^T] - mu mu^T

    "mean_std"  M = diag(sigma_t / sigma_s): Reinhard's transfer in RGB, ComfyUI ColorMatch's mean_std
    "mkl"       the Monge-Kantorovich linear map of Pitie & Kokaram 2007 ("The linear Monge-Kantorovitch linear colour mapping for
                example-based colour transfer"), M = Sigma_s^-1/2 (Sigma_s^1/2 Sigma_t Sigma_s^1/2)^1/2 Sigma_s^-1/2: the symmetric M with
                M Sigma_s M^T = Sigma_t.  Matrix square roots by numpy.linalg.eigh; eigenvalues are clipped at 0 before a root and at
                EIG_FLOOR before an inverse root, so a rank-deficient source covariance (a grey frame, whose channel variances pass the
                fallback test below) gives a finite M
    both        t = mu_t - M mu_s;  strength a:  M' = (1 - a) I + a M,  t' = a t
"""
import numpy as np

MODES = ("mean_std", "mkl")
SCOPES = ("frame", "clip")
# A frame whose source or target has a channel variance below this gets the mean shift alone.  A CHOICE of this project, not taken from any
# front end: a standard deviation of 1e-3, a quarter of a byte level (1 / 255 = 3.9e-3) -- below it a channel is flat to the eye and to the
# writer, and sigma_t / sigma_s would amplify rounding noise.
COLOR_MATCH_EPS = 1e-6
EIG_FLOOR = float(np.finfo(np.float64).eps)


def moments_of_image(arr):
    """The nine sums of an (H, W, 3) array of displayed colours in [0, 1], in float64 -> (sums (9,), n = H W).  For the target image."""
    s = np.asarray(arr, dtype=np.float64)
    if s.ndim != 3 or s.shape[2] != 3 or s.size == 0:
        raise ValueError(f"moments_of_image expects a non-empty (H, W, 3) array, got {s.shape}")
    s = s.reshape(-1, 3)
    s0, s1, s2 = s[:, 0], s[:, 1], s[:, 2]
    sums = np.array([s0.sum(), s1.sum(), s2.sum(), (s0 * s0).sum(), (s1 * s1).sum(), (s2 * s2).sum(), (s0 * s1).sum(), (s0 * s2).sum(),
                     (s1 * s2).sum()], dtype=np.float64)
    return sums, s.shape[0]


def mean_cov(sums, n):
    """(mu (3,), Sigma (3, 3)) of nine sums over n pixels, float64."""
    m = np.asarray(sums, dtype=np.float64) / float(n)
    mu = m[:3]
    second = np.array([[m[3], m[6], m[7]], [m[6], m[4], m[8]], [m[7], m[8], m[5]]])
    return mu, second - np.outer(mu, mu)


def _sqrt_spd(a, inverse=False):
    w, v = np.linalg.eigh((a + a.T) / 2)
    w = 1.0 / np.sqrt(np.maximum(w, EIG_FLOOR)) if inverse else np.sqrt(np.maximum(w, 0.0))
    return (v * w) @ v.T


def transform(src_sums, n_src, tgt_sums, n_tgt, mode, strength=1.0):
    """-> (M' (3, 3), t' (3,), fallback) in float64: the map that takes the source's colour statistics to the target's (see the module's
    docstring), at strength in [0, 1].  fallback=True: the frame gets the mean shift alone, M = I in both modes -- when a sum is not finite
    (a NaN in the frame; a channel whose shift is not finite then stays where it is), or when a source or target channel variance is below
    COLOR_MATCH_EPS (this project's choice, see there)."""
    if mode not in MODES:
        raise ValueError(f"color_match must be one of {MODES}, got {mode!r}")
    a = float(strength)
    src_sums, tgt_sums = np.asarray(src_sums, dtype=np.float64), np.asarray(tgt_sums, dtype=np.float64)
    eye = np.eye(3)
    finite = bool(np.isfinite(src_sums).all() and np.isfinite(tgt_sums).all())
    with np.errstate(all="ignore"):
        mu_s, cov_s = mean_cov(src_sums, n_src)
        mu_t, cov_t = mean_cov(tgt_sums, n_tgt)
    var_s, var_t = np.diag(cov_s), np.diag(cov_t)
    fallback = not finite or bool((var_s < COLOR_MATCH_EPS).any() or (var_t < COLOR_MATCH_EPS).any())
    if fallback:
        m = eye
        with np.errstate(all="ignore"):
            t = mu_t - mu_s
        t = np.where(np.isfinite(t), t, 0.0)
    else:
        if mode == "mean_std":
            m = np.diag(np.sqrt(var_t / var_s))
        else:
            root, inv = _sqrt_spd(cov_s), _sqrt_spd(cov_s, inverse=True)
            m = inv @ _sqrt_spd(root @ cov_t @ root) @ inv
            m = (m + m.T) / 2
        t = mu_t - m @ mu_s
    return (1.0 - a) * eye + a * m, a * t, fallback


def coefficients(maps):
    """[(M', t', fallback), ...] -> the (B, 12) float32 array ops.color_apply takes: row-major M', then t', rounded once."""
    return np.stack([np.concatenate([np.asarray(m, dtype=np.float64).reshape(9), np.asarray(t, dtype=np.float64)]) for m, t, _ in maps]).astype(np.float32)
