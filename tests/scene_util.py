"""numpy restatements of the whole-scene cloud-mask path (sentinel2.scene_windows / sc_scene_gather / CDModel.predict_scene)."""
import numpy as np


def padded_scene(bands, plan):
    """what predict() feeds the network: np.pad(..., "reflect") to multiples of 32"""
    return np.pad(bands, ((0, 0), tuple(plan.pad_rows), tuple(plan.pad_cols)), "reflect")


def gather_ref(bands, pad_rows, pad_cols, offsets, window, scale=1.0):
    """np.pad(reflect) + slicing + astype(float32) [* float32(scale)] -> (n, C, wh, ww)"""
    p = np.pad(bands, ((0, 0), tuple(pad_rows), tuple(pad_cols)), "reflect")
    wh, ww = window
    out = np.stack([p[:, r:r + wh, c:c + ww] for r, c in offsets]).astype(np.float32)
    assert out.shape[2:] == (wh, ww), "a window leaves the padded scene"
    return out * np.float32(scale) if scale != 1.0 else out


def coverage(plan, H, W):
    """how many cores hold each pixel of the (H, W) image"""
    cnt = np.zeros((H, W), dtype=np.int64)
    for (y0, y1, x0, x1), (dr, dc) in zip(plan.cores.tolist(), plan.dests.tolist()):
        if y1 > y0 and x1 > x0:
            assert dr >= 0 and dc >= 0 and dr + y1 - y0 <= H and dc + x1 - x0 <= W
            cnt[dr:dr + y1 - y0, dc:dc + x1 - x0] += 1
    return cnt


def paste_cores(per_window, plan, H, W):
    """per_window: (n, ..., wh, ww) results of the windows -> (..., H, W) with every core pasted at its destination"""
    out = np.zeros(per_window.shape[1:-2] + (H, W), dtype=per_window.dtype)
    for v, (y0, y1, x0, x1), (dr, dc) in zip(per_window, plan.cores.tolist(), plan.dests.tolist()):
        if y1 > y0 and x1 > x0:
            out[..., dr:dr + y1 - y0, dc:dc + x1 - x0] = v[..., y0:y1, x0:x1]
    return out
