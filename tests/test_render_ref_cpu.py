"""tests/render_ref.py, the float64 restatement that tests/test_gpu_render.py bounds csrc/render.hip
with: analytic values of the pixel function and of the cross-fade, the room the GPU module's
inputs leave a float32 kernel, the YUV4MPEG2 host path and the Python-side validation of
a2m.video (all of which run before anything touches a device)."""
import numpy as np
import pytest

import render_ref as R
import test_gpu_render as G

WHITE = (255, 255, 255)


def _one_line(y, half_width, W=16, H=9, x0=3.5, x1=11.5, rgb=(0, 0, 0), dtype=np.float64):
    kp = np.zeros((1, 1, 2, 2), np.float32)
    kp[0, 0, 0], kp[0, 0, 1] = (x0, x1), (y, y)
    idx, off = R.polyline_tables([(0, 1)])
    return R.render(kp, idx, off, [rgb], [[1, 0, 1, 0]], half_width, WHITE, W, H, dtype)[0]


# ------------------------------------------------------------------------------ the pixel function
def test_horizontal_line_through_pixel_centres():
    img = _one_line(4.5, 1.5)                    # pixel row 4; columns 3..11 lie on the segment
    for row in (3, 4, 5):                        # distance 0 and 1: c = clamp(2 - d) = 1
        assert (img[:, row, 3:12] == 0).all(), row
    assert (img[:, 2] == 255).all() and (img[:, 6] == 255).all()     # distance 2: c = 0, background
    assert (img[:, 0] == 255).all() and (img[:, 8] == 255).all()
    # round caps: two pixels past the end on the line's own row d = 2 -> background, one pixel d = 1
    assert (img[:, 4, 1] == 255).all() and (img[:, 4, 2] == 0).all()
    assert (img[:, 4, 13] == 255).all() and (img[:, 4, 12] == 0).all()


def test_half_coverage_at_distance_one():
    img = _one_line(4.5, 1.0)                    # c = clamp(1.5 - 1) = 0.5 -> 127.5 -> 128
    assert (img[:, 4, 3:12] == 0).all()
    assert (img[:, 3, 3:12] == 128).all() and (img[:, 5, 3:12] == 128).all()
    assert (img[:, 2] == 255).all() and (img[:, 6] == 255).all()
    red = _one_line(4.5, 1.0, rgb=(255, 0, 0))
    assert (red[0, 3, 3:12] == 255).all() and (red[1, 3, 3:12] == 128).all()


def test_zero_length_segment_is_a_point_and_non_finite_segments_are_skipped():
    dot = _one_line(4.5, 1.0, x0=7.5, x1=7.5)
    assert dot[0, 4, 7] == 0 and dot[0, 4, 6] == 128 and dot[0, 3, 7] == 128 and dot[0, 4, 5] == 255
    assert dot[0, 3, 6] == 255 - round(255 * (1.5 - np.sqrt(2)))
    assert (_one_line(4.5, 1.0, x1=np.nan) == 255).all()
    assert (_one_line(np.inf, 1.0) == 255).all()


def test_joint_has_no_darker_fringe_and_draw_order_wins():
    """Two segments of one polyline share one coverage (their union); a later polyline paints over."""
    kp = np.array([[[[2.5, 8.5, 8.5], [4.5, 4.5, 0.5]]]], np.float32)
    idx, off = R.polyline_tables([(0, 1, 2)])
    half = R.render(kp, idx, off, [(0, 0, 0)], [[1, 0, 1, 0]], 0.25, WHITE, 12, 8)[0]
    assert half[0, 4, 8] == 64                   # c = 0.75 once, not 1 - 0.25^2
    idx2, off2 = R.polyline_tables([(0, 1), (1, 2)])
    two = R.render(kp, idx2, off2, [(0, 0, 0), (0, 0, 0)], [[1, 0, 1, 0]], 0.25, WHITE, 12, 8)[0]
    assert two[0, 4, 8] == 16                    # 255 * 0.25 * 0.25 = 15.94
    over = R.render(kp, idx2, off2, [(0, 0, 0), (255, 0, 0)], [[1, 0, 1, 0]], 1.5, WHITE, 12, 8)[0]
    assert tuple(over[:, 4, 8]) == (255, 0, 0) and tuple(over[:, 4, 4]) == (0, 0, 0)


def test_poses_are_drawn_in_order_with_their_own_transform():
    kp = np.zeros((1, 2, 2, 2), np.float32)
    kp[0, :, 0], kp[0, :, 1] = (1.5, 6.5), (2.5, 2.5)
    idx, off = R.polyline_tables([(0, 1)])
    xf = [[1, 0, 1, 0], [1, 2, 1, 0]]           # pose 1 two pixels to the right
    a = R.render(kp, idx, off, [(10, 20, 30)], xf, 0.5, WHITE, 12, 5)[0]
    assert tuple(a[:, 2, 1]) == (10, 20, 30) and tuple(a[:, 2, 8]) == (10, 20, 30) and a[0, 2, 10] == 255
    xf2 = [[2, 0.5, 2, 0.5], [1, 0, 1, 0]]      # pose 0: (3.5, 5.5) - (13.5, 5.5)
    b = R.render(kp, idx, off, [(0, 0, 0)], xf2, 0.5, WHITE, 16, 8)[0]
    assert b[0, 5, 3] == 0 and b[0, 5, 13] == 0 and b[0, 2, 3] == 0 and b[0, 2, 10] == 255


# ------------------------------------------------------------------------------ room for float32
@pytest.mark.parametrize('canvas', G.CANVASES, ids=lambda c: '%dx%d' % c)
@pytest.mark.parametrize('name', G.CASE_NAMES)
def test_gpu_inputs_leave_a_float32_kernel_room(name, canvas):
    """The restatement in float32 differs from float64 by at most 1, on at most a tenth of the
    share of a frame's bytes that the GPU test allows the kernel."""
    case = G.render_case(name, canvas)
    ref = G.reference(case, canvas)
    f32 = G.reference(case, canvas, np.float32)
    worst, count = G.frame_diffs(f32, ref)
    assert worst.max() <= 1
    assert (count <= 0.1 * G.MAX_DIFF_SHARE * ref[0].size).all(), count
    assert case['kp'].shape[0] == G.N and case['kp'].shape[3] == G.K
    if name != 'outside':
        drawn = (ref != 255).any(1).reshape(G.N, -1).mean(1)
        assert (drawn > 0.02).all(), drawn         # every frame really draws something


def test_gpu_cases_are_what_they_claim():
    W, H = G.CANVASES[0]
    assert (G.reference(G.render_case('outside', (W, H)), (W, H)) == 255).all()
    kp = G.render_case('crossing', (W, H))['kp']
    assert kp[:, :, 0].min() < 0 and kp[:, :, 0].max() > W and kp[:, :, 1].min() < 0 and kp[:, :, 1].max() > H
    a, b = kp[:, 0, :, 1:3], kp[:, 0, :, 2:4]           # two segments of the right body line
    assert ((np.minimum(a[:, 0], b[:, 0]) < 64) & (np.maximum(a[:, 0], b[:, 0]) > 64)).any()
    kp = G.render_case('nan', (W, H))['kp']
    assert not np.isfinite(kp).all() and np.isfinite(kp).mean() > 0.98
    kp = G.render_case('zero_length', (W, H))['kp']
    assert (kp[..., 7] == kp[..., 8]).all()
    two = G.render_case('two_poses', (W, H))
    assert two['kp'].shape[1] == 2 and two['offsets'] is not None
    # the second pose paints over the first somewhere: swapping them changes the picture
    swapped = dict(two, kp=two['kp'][:, ::-1].copy(), offsets=two['offsets'][::-1])
    assert (G.reference(two, (W, H)) != G.reference(swapped, (W, H))).any()


# ------------------------------------------------------------------------------ the cross-fade
@pytest.mark.parametrize('T,overlap', [(8, 1), (8, 4), (64, 16), (7, 3)])
def test_blend_weights_sum_to_one_over_every_overlap(T, overlap):
    n, h = 4, T - overlap
    total = np.zeros((n - 1) * h + T)
    for k in range(n):
        total[k * h:k * h + T] += R.blend_weights(T, overlap, n, k)
    assert np.array_equal(total, np.ones_like(total))
    w = R.blend_weights(T, overlap, n, 1)
    assert w[0] == 0.5 / overlap and w[T - 1] == 0.5 / overlap and (w[overlap:T - overlap] == 1).all()
    assert (R.blend_weights(T, overlap, n, 0)[:overlap] == 1).all()
    assert (R.blend_weights(T, overlap, n, n - 1)[T - overlap:] == 1).all()


def test_blend_without_overlap_is_concatenation():
    win, mean, std = G.blend_inputs(3)
    out, cover = R.blend(win, 0)
    assert np.array_equal(out, win.reshape(-1, G.FD).astype(np.float64)) and (cover == 1).all()
    out, _ = R.blend(win, 0, mean, std)
    assert np.array_equal(out, win.reshape(-1, G.FD).astype(np.float64) * std + mean)
    out, cover = R.blend(win, 4)
    assert out.shape == (2 * 4 + 8, G.FD) and (cover == 2).sum() == 8
    assert np.array_equal(out[:4], win[0, :4]) and np.array_equal(out[-4:], win[2, 4:])
    w64 = win.astype(np.float64)
    assert np.allclose(out[4], (3.5 * w64[0, 4] + 0.5 * w64[1, 0]) / 4, rtol=1e-14, atol=0)


# ------------------------------------------------------------------------------ YUV4MPEG2, PPM
def test_y4m_round_trip(tmp_path):
    from a2m import video as V
    rng = np.random.default_rng(3)
    frames = rng.integers(0, 256, (5, 3, 6, 10), dtype=np.uint8)
    fn = tmp_path / 'clip.y4m'
    V.write_y4m(str(fn), frames)
    raw = fn.read_bytes()
    header = b'YUV4MPEG2 W10 H6 F30000:2002 Ip A1:1 C444\n'
    assert raw.startswith(header) and len(raw) == len(header) + 5 * (6 + 180)
    hdr, planes = R.parse_y4m(str(fn))
    assert hdr == {'W': '10', 'H': '6', 'F': '30000:2002', 'I': 'p', 'A': '1:1', 'C': '444'}
    assert planes.shape == (5, 3, 6, 10) and np.array_equal(planes, frames)
    with V.Y4MWriter(str(tmp_path / 'chunks.y4m'), 10, 6, fps=(15, 1)) as w:
        w.write(frames[:2])
        w.write(frames[2:])
        with pytest.raises(ValueError):
            w.write(frames[:, :, :5])
    hdr, planes = R.parse_y4m(str(tmp_path / 'chunks.y4m'))
    assert hdr['F'] == '15:1' and np.array_equal(planes, frames)
    V.write_y4m(str(tmp_path / 'empty.y4m'), frames[:0])
    assert R.parse_y4m(str(tmp_path / 'empty.y4m'))[1].shape == (0, 3, 6, 10)


def test_ppm_and_palette_conversion(tmp_path):
    from a2m import video as V
    frame = np.arange(3 * 2 * 4, dtype=np.uint8).reshape(3, 2, 4)
    V.write_ppm(str(tmp_path / 'f.ppm'), frame)
    raw = (tmp_path / 'f.ppm').read_bytes()
    assert raw[:11] == b'P6\n4 2\n255\n' and raw[11:14] == bytes([0, 8, 16]) and len(raw) == 11 + 24
    ycc = V.rgb_to_ycbcr([(255, 255, 255), (0, 0, 0), (255, 0, 0), (0, 0, 255), (128, 128, 128)])
    assert ycc.tolist() == [[235, 128, 128], [16, 128, 128], [81, 90, 240], [41, 240, 110], [126, 128, 128]]


# ------------------------------------------------------------------------------ validation, tables
def test_draw_groups():
    from a2m import video as V
    from a2m.skeleton import PARENTS
    assert len(V.REFERENCE_POLYLINES) == len(V.REFERENCE_COLORS) == 14
    assert V.REFERENCE_POLYLINES[:4] == ((7, 8), (7, 9), (1, 2, 3, 31), (4, 5, 6, 10))
    assert [l[0] for l in V.REFERENCE_POLYLINES[4:]] == [10] * 5 + [31] * 5
    assert V.REFERENCE_POLYLINES[4] == (10, 11, 12, 13, 14) and V.REFERENCE_POLYLINES[8][-1] == 30
    assert V.REFERENCE_POLYLINES[9] == (31, 29, 30, 31, 32) and V.REFERENCE_POLYLINES[13] == (31, 45, 46, 47, 48)
    assert len(V.SKELETON_POLYLINES) == len(V.SKELETON_COLORS) == 51
    assert all(PARENTS[j] == p for p, j in V.SKELETON_POLYLINES)
    assert abs(V.REFERENCE_LINE_WIDTH - 10.4167) < 1e-4


def test_python_side_validation():
    from a2m import video as V
    kp = np.zeros((2, 2, 52), np.float32)
    with pytest.raises(ValueError, match='outside'):
        V.render_poses(kp[:, :, :31])                               # the draw groups reach keypoint 48
    with pytest.raises(ValueError, match='outside'):
        V.render_poses(kp, polylines=[(0, -1)])
    with pytest.raises(ValueError, match='at least 2'):
        V.render_poses(kp, polylines=[(0, 1), (3,)])
    with pytest.raises(ValueError, match='colors'):
        V.render_poses(kp, polylines=[(0, 1)], colors=[(0, 0, 0), (1, 1, 1)])
    for bad in (kp[0], kp.reshape(2, 52, 2), np.zeros((2, 1, 3, 52), np.float32)):
        with pytest.raises(ValueError, match='keypoints must be'):
            V.render_poses(bad)
    with pytest.raises(ValueError, match='offsets'):
        V.render_poses(kp, offsets=[(0, 0), (1, 1)])
    with pytest.raises(ValueError, match='line_width'):
        V.render_poses(kp, line_width=-1.0)
    with pytest.raises(ValueError, match='.y4m'):
        V.save_side_by_side_video('tmp', kp, kp, 'out.mp4')
    with pytest.raises(ValueError, match='.y4m'):
        V.save_pose_video(kp, 'out.avi')
    with pytest.raises(NotImplementedError):
        V.draw_side_by_side_poses('photo.jpg', kp[0], kp[0])
