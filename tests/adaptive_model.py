"""Host model of adaptive sampling (atr_render_start_adaptive), computed from oracle renders alone.

Every pixel's outputs after any number of adaptive passes are the oracle's one-shot render at that
pixel's own sample count, so whole-frame oracle renders at the schedule's cumulative totals are all
the model needs: the running sum of a pixel at total T is not kept by the oracle, but the rule only
uses the two means (the oracle's f32 rgb at the totals before and after the pass)."""
import numpy as np

FLAG = np.uint32(0x80000000)


def converged(mean_before, mean_after, tolerance):
    """The stopping rule of atray.h in float32, every operation separately rounded, in its order."""
    a = mean_before.astype(np.float32)
    m = mean_after.astype(np.float32)
    tol = np.float32(tolerance)
    with np.errstate(invalid="ignore"):
        d = (np.abs(m[..., 0] - a[..., 0]) + np.abs(m[..., 1] - a[..., 1])) + np.abs(m[..., 2] - a[..., 2])
        l = ((m[..., 0] + m[..., 1]) + m[..., 2]) + np.float32(0.01)
        return d < tol * l, d, tol * l


def block_ids(W, H, pixels=None, waves=1):
    """Block id per pixel, (H, W) int64: the 8x8 cells of the image grid, or with a `waves`-wave cell
    plan their bands of 8 / waves rows. -1 outside `pixels` (flat pixel indices; None = all)."""
    y, x = np.mgrid[0:H, 0:W]
    rows = 8 // waves
    ids = ((y // 8) * ((W + 7) // 8) + x // 8) * waves + (y % 8) // rows
    if pixels is not None:
        own = np.zeros(W * H, bool)
        own[np.asarray(pixels)] = True
        ids = np.where(own.reshape(H, W), ids, -1)
    return ids


def run(means, passes, tolerance, blocks):
    """means: {total: (H, W, 3) f32 oracle rgb}; blocks: block_ids(). Per pass: the expected count map
    with flags ((H, W) u32; 0 outside the blocks) and the four atr_render_adaptive_info values."""
    owned = blocks >= 0
    count = np.zeros(blocks.shape, np.uint32)
    out, first = [], 0
    for n in passes:
        live = owned & ((count == np.uint32(first)) if first else np.ones_like(owned))
        per_block = np.bincount(blocks[live], minlength=int(blocks.max()) + 1)
        groups = int(((per_block * n + 63) // 64).sum())
        conv = np.zeros_like(live)
        if first:
            conv = live & converged(means[first], means[first + n], tolerance)[0]
        count = np.where(live, np.uint32(first + n) | np.where(conv, FLAG, np.uint32(0)), count).astype(np.uint32)
        out.append((count.copy(), (int(live.sum()), int((per_block > 0).sum()), groups, int(live.sum() - conv.sum()))))
        first += n
    return out


def threshold_margin(means, passes, tolerance):
    """Smallest |d - tolerance x l| / ulp over every tested pixel and pass: the model is only as
    good as its distance from the comparison's threshold."""
    worst, first = np.inf, 0
    for n in passes:
        if first:
            _, d, tl = converged(means[first], means[first + n], tolerance)
            ulp = np.spacing(np.maximum(np.abs(d), np.abs(tl)).astype(np.float32))
            worst = min(worst, float(np.nanmin(np.abs(d - tl) / ulp)))
        first += n
    return worst
