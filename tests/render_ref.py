"""Restatements that pin csrc/render.hip: the pixel function of a2m_render_poses_u8 and the
cross-fade of a2m_track_blend_f32 in float64 numpy, and a YUV4MPEG2 parser.

render(...) takes the same arrays as the C entry point.  dtype=np.float32 evaluates the same
formulas in single precision: tests/test_render_ref_cpu.py uses it to show that the inputs of
tests/test_gpu_render.py sit far enough from rounding boundaries to leave a float32 kernel room.
"""
import numpy as np


def polyline_tables(polylines):
    """[(i0, i1, ...), ...] -> (poly_idx int32, poly_off int32 [L+1])."""
    idx = np.array([i for line in polylines for i in line], np.int32)
    off = np.concatenate([[0], np.cumsum([len(line) for line in polylines])]).astype(np.int32)
    return idx, off


def _segment_dist2(qx, qy, a, b, dt):
    """Squared distance from the pixel centres (qx [W], qy [H]) to segment a-b -> [H, W]."""
    ex, ey = dt(b[0] - a[0]), dt(b[1] - a[1])
    len2 = dt(ex * ex + ey * ey)
    rx, ry = (qx - a[0])[None, :], (qy - a[1])[:, None]
    sx, sy = (qx - b[0])[None, :], (qy - b[1])[:, None]
    dot = rx * ex + ry * ey
    cr = rx * ey - ry * ex
    da, db = rx * rx + ry * ry, sx * sx + sy * sy
    with np.errstate(divide='ignore', invalid='ignore'):
        dm = cr * cr / len2 if len2 > 0 else np.zeros_like(da)
    return np.where(dot <= 0, da, np.where(dot >= len2, db, dm)).astype(dt)


def coverage(pts, line, reach, W, H, dt=np.float64):
    """c [H, W] of one polyline (keypoint indices `line`) over pixel-space points pts [2, K]."""
    qx, qy = np.arange(W, dtype=dt) + dt(0.5), np.arange(H, dtype=dt) + dt(0.5)
    d2 = np.full((H, W), np.inf, dt)
    for i0, i1 in zip(line[:-1], line[1:]):
        a, b = pts[:, i0], pts[:, i1]
        if not (np.isfinite(a).all() and np.isfinite(b).all()):
            continue
        d2 = np.minimum(d2, _segment_dist2(qx, qy, a, b, dt))
    return np.clip(dt(reach) - np.sqrt(d2), dt(0), dt(1)).astype(dt)


def render(kp, poly_idx, poly_off, poly_rgb, xform, half_width_px, bg, W, H, dtype=np.float64):
    """kp [N, P, 2, K] float32, xform [P, 4] float32 -> uint8 [N, 3, H, W]."""
    dt = np.dtype(dtype).type
    kp = np.asarray(kp, np.float32)
    N, P, _, K = kp.shape
    xf = np.asarray(xform, np.float32).astype(dt)
    rgb = np.asarray(poly_rgb, np.uint8).reshape(-1, 3).astype(dt)
    lines = [list(poly_idx[poly_off[l]:poly_off[l + 1]]) for l in range(len(poly_off) - 1)]
    reach = dt(np.float32(half_width_px)) + dt(0.5)
    out = np.empty((N, 3, H, W), np.uint8)
    with np.errstate(invalid='ignore'):
        for n in range(N):
            v = np.empty((3, H, W), dt)
            v[:] = np.asarray(bg, np.uint8).astype(dt)[:, None, None]
            for p in range(P):
                pts = np.stack([xf[p, 0] * kp[n, p, 0].astype(dt) + xf[p, 1],
                                xf[p, 2] * kp[n, p, 1].astype(dt) + xf[p, 3]]).astype(dt)
                for l, line in enumerate(lines):
                    c = coverage(pts, line, reach, W, H, dt)
                    v = (v * (dt(1) - c) + rgb[l][:, None, None] * c).astype(dt)
            out[n] = np.floor(v + dt(0.5)).astype(np.uint8)
    return out


def blend_weights(T, overlap, n, k):
    """Weight of every frame of window k among n windows (float64 [T])."""
    j = np.arange(T, dtype=np.float64)
    w = np.ones(T)
    if overlap:
        if k > 0:
            w[:overlap] = (j[:overlap] + 0.5) / overlap
        if k < n - 1:
            w[T - overlap:] = (T - j[T - overlap:] - 0.5) / overlap
    return w


def blend(win, overlap, mean=None, std=None):
    """win [n, T, Fd] -> float64 [(n-1)(T-overlap)+T, Fd]; also the per-frame window count."""
    win = np.asarray(win, np.float64)
    n, T, Fd = win.shape
    h = T - overlap
    out = np.zeros(((n - 1) * h + T, Fd))
    cover = np.zeros((n - 1) * h + T, np.int64)
    for k in range(n):
        out[k * h:k * h + T] += blend_weights(T, overlap, n, k)[:, None] * win[k]
        cover[k * h:k * h + T] += 1
    if mean is not None:
        out = out * np.asarray(std, np.float64) + np.asarray(mean, np.float64)
    return out, cover


def parse_y4m(path):
    """-> (header dict {'W','H','F','I','A','C'}, frames uint8 [n, 3, H, W]) of a C444 file."""
    with open(path, 'rb') as f:
        data = f.read()
    end = data.index(b'\n')
    tokens = data[:end].split(b' ')
    assert tokens[0] == b'YUV4MPEG2', tokens[0]
    hdr = {t[:1].decode(): t[1:].decode() for t in tokens[1:]}
    W, H = int(hdr['W']), int(hdr['H'])
    assert hdr['C'] == '444', hdr
    frames, pos, size = [], end + 1, 3 * W * H
    while pos < len(data):
        assert data[pos:pos + 6] == b'FRAME\n', data[pos:pos + 6]
        pos += 6
        assert pos + size <= len(data), 'truncated frame'
        frames.append(np.frombuffer(data, np.uint8, size, pos).reshape(3, H, W))
        pos += size
    return hdr, (np.stack(frames) if frames else np.empty((0, 3, H, W), np.uint8))
