"""numpy restatement of the shadow post-pass (include/trgl.h, steps 1-8 of trgl_shadow_mask_image, and Modulate): vectorised over the
pixels, with every multiply and add written out in the order the header fixes - numpy's float64 `*`, `+`, `/` are IEEE operations,
one rounding each, no fusing.  The oracle of the host path (tests/test_shadow.py) and of the kernels (tests/test_shadow_gpu.py)."""
import numpy as np


def shadow_mask(depth, M, zmap, bias, darkness, pcf_radius):
    depth = np.asarray(depth, np.float64)
    zmap = np.asarray(zmap, np.float64)
    M = np.asarray(M, np.float64).reshape(4, 4)
    h, w = depth.shape
    map_h, map_w = zmap.shape
    out = np.full((h, w), 255, np.uint8)
    if h == 0 or w == 0:
        return out
    with np.errstate(all="ignore"):
        z = depth
        live = np.isfinite(z)                                                   # 1
        ys, xs = np.mgrid[0:h, 0:w]
        p = (xs.astype(np.float64) + 0.5, ys.astype(np.float64) + 0.5, z, np.ones_like(z))   # 2
        q = []
        for r in range(4):
            s = np.zeros_like(z)
            for c in range(4):
                s = s + M[r, c] * p[c]
            q.append(s)
        live &= q[3] > 1e-12                                                    # 3 (False for a NaN)
        s = [q[k] / q[3] for k in range(3)]                                     # 4
        live &= np.isfinite(s[0]) & np.isfinite(s[1]) & np.isfinite(s[2])
        live &= ~((s[2] < -1.0) | (s[2] > 1.0))                                 # 5
        live &= (s[0] >= 0.0) & (s[0] < float(map_w)) & (s[1] >= 0.0) & (s[1] < float(map_h))   # 6
        ix = np.where(live, s[0], 0.0).astype(np.int64)                         # 7: truncation, of values in [0, map_w)
        iy = np.where(live, s[1], 0.0).astype(np.int64)
        limit = s[2] - bias
        r = int(pcf_radius)
        occluded = np.zeros((h, w), np.int64)
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                tx, ty = ix + dx, iy + dy
                inside = (tx >= 0) & (tx < map_w) & (ty >= 0) & (ty < map_h)
                tap = zmap[np.clip(ty, 0, map_h - 1), np.clip(tx, 0, map_w - 1)]
                occluded += (inside & (tap < limit)).astype(np.int64)
        total = (2 * r + 1) * (2 * r + 1)
        factor = 1.0 - (occluded.astype(np.float64) / np.float64(total)) * np.float64(darkness)   # 8
        byte = (255.0 * factor).astype(np.uint8)
    out[live] = byte[live]
    return out


def modulate(img, mask):
    img = np.asarray(img, np.uint8)
    h, w, bpp = img.shape
    f = np.asarray(mask, np.uint8).reshape(h, w, 1).astype(np.float64) / 255.0
    out = img.copy()
    nc = min(bpp, 3)
    out[..., :nc] = np.minimum(255.0, img[..., :nc].astype(np.float64) * f).astype(np.uint8)
    return out
