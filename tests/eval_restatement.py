"""Float64 restatement of the reference's validation metrics (Utils/Eval_utils.py:11-48,54-66,101-106), numpy only.

The reference calls scikit-image 0.19.3 (structural_similarity) and opencv-python 4.8.1.78 (cvtColor, PSNR).  Neither is a
dependency of this project, so what they compute is written down here, one line per step, and pinned by recorded fixtures
(tests/golden/eval_metrics.*; tools/gen_golden_eval.py).  Parity is therefore unpinned to the dependency: the grey-conversion
constants in particular are OpenCV's as read from its source, not as run.

This is the oracle of n3dt.eval_utils.  It shares no code and no method with the kernel: the window means below are direct
means over sliding windows, not running integer sums.
"""
import numpy as np

GRAY_SHIFT = 15
BY15, GY15, RY15 = 3735, 19235, 9798   # OpenCV's 15-bit fixed-point weights of B, G, R
K1, K2, DATA_RANGE, WIN = 0.01, 0.03, 255.0, 7
C1, C2 = (K1 * DATA_RANGE) ** 2, (K2 * DATA_RANGE) ** 2
DBL_EPSILON = 2.220446049250313e-16


def quantise(x):
    """float32 [...] -> uint8: `(x * 255).astype(np.uint8)` -- a float32 multiply, then truncation -- with the project's
    definition outside [0, 1]: clamp to [0, 255], NaN -> 0 (numpy's cast is undefined there)."""
    x = np.asarray(x, dtype=np.float32)
    v = x * np.float32(255.0)
    v = np.where(np.isnan(v), np.float32(0.0), v)
    return np.clip(v, np.float32(0.0), np.float32(255.0)).astype(np.uint8)


def gray_bgr(u8):
    """cv2.cvtColor(u8, COLOR_BGR2GRAY) on uint8 [H,W,3]: channel 0 is weighted as B, whatever the image holds there."""
    c = u8.astype(np.int64)
    return ((c[..., 0] * BY15 + c[..., 1] * GY15 + c[..., 2] * RY15 + (1 << (GRAY_SHIFT - 1))) >> GRAY_SHIFT).astype(np.uint8)


def _window_mean(a):
    return np.lib.stride_tricks.sliding_window_view(a, (WIN, WIN)).mean((-1, -2))


def ssim_u8(g1, g2):
    """skimage.metrics.structural_similarity(g1, g2) with every default on uint8 [H,W]: float64, 7x7 uniform window,
    data_range 255, sample covariance, the mean of S over the image cropped by 3 on every side (exactly the positions
    whose window lies inside the image, so the filter's border mode never matters)."""
    x, y = g1.astype(np.float64), g2.astype(np.float64)
    cov_norm = WIN * WIN / (WIN * WIN - 1.0)
    ux, uy = _window_mean(x), _window_mean(y)
    uxx, uyy, uxy = _window_mean(x * x), _window_mean(y * y), _window_mean(x * y)
    vx = cov_norm * (uxx - ux * ux)
    vy = cov_norm * (uyy - uy * uy)
    vxy = cov_norm * (uxy - ux * uy)
    a1, a2 = 2.0 * ux * uy + C1, 2.0 * vxy + C2
    b1, b2 = ux * ux + uy * uy + C1, vx + vy + C2
    s = (a1 * a2) / (b1 * b2)
    return float(s.mean(dtype=np.float64))


def psnr_u8(u1, u2):
    """cv2.PSNR(u1, u2) on uint8 [H,W,3]: 20 log10(255 / (sqrt(SSE / (H W 3)) + DBL_EPSILON)); finite for identical images."""
    d = u1.astype(np.int64) - u2.astype(np.int64)
    sse = float((d * d).sum())
    return float(20.0 * np.log10(255.0 / (np.sqrt(sse / d.size) + DBL_EPSILON)))


def metrics(pred, gt):
    """pred, gt float32 [3,H,W] (one image each, planar like the renderer's output) -> (ssim, psnr) as the reference's
    calc_eval_metrics forms them: permute to [H,W,3], quantise, grey-convert for SSIM, colour bytes for PSNR."""
    u1 = quantise(np.transpose(np.asarray(pred), (1, 2, 0)))
    u2 = quantise(np.transpose(np.asarray(gt), (1, 2, 0)))
    return ssim_u8(gray_bgr(u1), gray_bgr(u2)), psnr_u8(u1, u2)


def batch_metrics(pred, gt):
    """[B,3,H,W] -> (ssim [B], psnr [B]) float64"""
    r = [metrics(p, g) for p, g in zip(np.asarray(pred), np.asarray(gt))]
    return np.array([a for a, _ in r], dtype=np.float64), np.array([b for _, b in r], dtype=np.float64)
