"""csrc/render.hip on the GPU against tests/render_ref.py: the rasteriser a2m_render_poses_u8
through a2m.video.render_poses, the stitcher a2m_track_blend_f32, generate_track and the YUV4MPEG2
writer.

Rasteriser criterion, per frame: no byte differs from the float64 restatement by more than 1, and
bytes that differ by 1 are at most 0.1 % of the frame's bytes.  The inputs come from a fixed seed
on a 1/16-pixel grid with integer offsets and scale 1: differences and products of such
coordinates below 128 are exact in float32, so what is left of the float32 error is relative to
the distance itself (about 1e-7 of 2-3 pixels), and tests/test_render_ref_cpu.py asserts that the
restatement evaluated in float32 differs from float64 on at most a tenth of that cap.
"""
import functools

import numpy as np
import pytest

import render_ref as R

pytestmark = pytest.mark.gpu

N, K = 3, 52
CANVASES = ((96, 40), (97, 41))     # W % 4 == 0: aligned dword rows; W % 4 != 0: the byte path
HALF_WIDTH = 1.5
MAX_DIFF_SHARE = 1e-3               # of a frame's bytes, each off by at most 1
CASE_NAMES = ('generic', 'outside', 'crossing', 'zero_length', 'nan', 'two_poses', 'skeleton',
              'hairline')


def _grid(a):
    return (np.round(np.asarray(a, np.float64) * 16) / 16).astype(np.float32)


def render_case(name, canvas):
    """-> dict(kp [N, P, 2, K] float32, polylines, colors, offsets or None, half_width)."""
    from a2m import video as V
    W, H = canvas
    rng = np.random.default_rng(20240 + CASE_NAMES.index(name))
    P = 2 if name == 'two_poses' else 1
    kp = np.empty((N, P, 2, K), np.float64)
    kp[:, :, 0] = rng.uniform(2, W - 2, (N, P, K))
    kp[:, :, 1] = rng.uniform(2, H - 2, (N, P, K))
    case = dict(polylines=V.REFERENCE_POLYLINES, colors=V.REFERENCE_COLORS, offsets=None,
                half_width=HALF_WIDTH)
    if name == 'outside':
        kp += 1000.0
    elif name == 'crossing':       # segments across the 64-pixel tile border, the 4- and 16-row
        kp[:, :, 0] = rng.uniform(-30, W + 30, (N, P, K))   # borders and every canvas edge
        kp[:, :, 1] = rng.uniform(-20, H + 20, (N, P, K))
    elif name == 'zero_length':
        kp[:, :, :, 8] = kp[:, :, :, 7]             # head line (7, 8) is a point
        kp[:, :, :, 11:15] = kp[:, :, :, 10:11]     # a whole finger collapses onto the hand root
        kp[:, :, :, 2] = kp[:, :, :, 1]             # a point inside a longer polyline
    elif name == 'nan':
        kp[0, 0, 0, 5] = np.nan                     # breaks two segments of the left body line
        kp[1, 0, 1, 31] = np.inf                    # every right-hand finger loses its first segments
        kp[2, 0, :, 7] = np.nan                     # both head lines: no valid segment at all
    elif name == 'two_poses':
        case['offsets'] = ((0, 0), (7, -3))
    elif name == 'skeleton':
        case['polylines'], case['colors'] = V.SKELETON_POLYLINES, V.SKELETON_COLORS
    elif name == 'hairline':
        case['half_width'] = 0.0
    case['kp'] = _grid(kp)
    return case


def reference(case, canvas, dtype=np.float64):
    W, H = canvas
    idx, off = R.polyline_tables(case['polylines'])
    P = case['kp'].shape[1]
    xf = np.tile(np.array([1, 0, 1, 0], np.float32), (P, 1))
    if case['offsets'] is not None:
        xf[:, 1], xf[:, 3] = np.asarray(case['offsets'], np.float32).T
    return R.render(case['kp'], idx, off, case['colors'], xf, case['half_width'], (255, 255, 255), W, H,
                    dtype)


@functools.lru_cache(maxsize=None)
def _ref64(name, canvas):
    ref = reference(render_case(name, canvas), canvas)
    ref.setflags(write=False)
    return ref


def frame_diffs(got, ref):
    """Per frame: (largest byte difference, number of differing bytes)."""
    d = np.abs(got.astype(np.int16) - ref.astype(np.int16)).reshape(len(ref), -1)
    return d.max(1) if d.size else d.sum(1), (d != 0).sum(1)


def _render(case, canvas, **kw):
    import torch
    from a2m import video as V
    return V.render_poses(torch.from_numpy(case['kp']).cuda(), case['polylines'], case['colors'],
                          canvas=canvas, scale=1.0, line_width=2 * case['half_width'],
                          offsets=case['offsets'], **kw)


@pytest.mark.parametrize('canvas', CANVASES, ids=lambda c: '%dx%d' % c)
@pytest.mark.parametrize('name', CASE_NAMES)
def test_rasteriser_matches_float64(name, canvas):
    case = render_case(name, canvas)
    got = _render(case, canvas).cpu().numpy()
    ref = _ref64(name, canvas)
    assert got.shape == ref.shape == (N, 3, canvas[1], canvas[0])
    worst, count = frame_diffs(got, ref)
    print(f'{name} {canvas}: largest difference {worst.tolist()}, differing bytes {count.tolist()} '
          f'of {ref[0].size}')
    if name == 'outside':
        assert (got == 255).all() and (ref == 255).all()
    else:
        assert (ref != 255).any(), 'the case draws nothing'
    assert worst.max() <= 1
    assert (count <= MAX_DIFF_SHARE * ref[0].size).all()


def test_numpy_in_numpy_out_and_three_dim_input():
    from a2m import video as V
    case = render_case('generic', CANVASES[0])
    got = V.render_poses(case['kp'][:, 0], canvas=CANVASES[0], scale=1.0, line_width=2 * HALF_WIDTH)
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8
    worst, count = frame_diffs(got, _ref64('generic', CANVASES[0]))
    assert worst.max() <= 1 and (count <= MAX_DIFF_SHARE * got[0].size).all()


def test_empty_batch_and_out_argument():
    import torch
    from a2m import video as V
    W, H = CANVASES[1]
    empty = V.render_poses(torch.empty(0, 2, K, device='cuda'), canvas=(W, H), scale=1.0)
    assert tuple(empty.shape) == (0, 3, H, W) and empty.dtype == torch.uint8
    case = render_case('generic', (W, H))
    out = torch.full((N, 3, H, W), 7, dtype=torch.uint8, device='cuda')
    back = _render(case, (W, H), out=out)
    assert back.data_ptr() == out.data_ptr()
    assert torch.equal(out, _render(case, (W, H)))
    with pytest.raises(ValueError):
        _render(case, (W, H), out=out[:, :, :, :-1])


def test_graph_replay_gives_the_same_bytes():
    import torch
    case = render_case('crossing', CANVASES[0])
    other = render_case('generic', CANVASES[0])
    kp = torch.from_numpy(case['kp']).cuda()
    from a2m import video as V
    kw = dict(canvas=CANVASES[0], scale=1.0, line_width=2 * HALF_WIDTH)
    eager = V.render_poses(kp, **kw)
    out = torch.zeros_like(eager)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        V.render_poses(kp, out=out, **kw)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    kp.copy_(torch.from_numpy(other['kp']))       # the replay reads the static input again
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, V.render_poses(kp, **kw))


# ------------------------------------------------------------------------------ a2m_track_blend_f32
T, FD = 8, 104


def blend_inputs(n):
    """Positive windows, mean and std: the sums of an overlap then carry no cancellation, which is
    what the 4-ulp bound (two products, one sum, one multiply-add) assumes."""
    rng = np.random.default_rng(77 + n)
    win = rng.uniform(0.25, 4.0, (n, T, FD)).astype(np.float32)
    mean = rng.uniform(0.5, 300.0, FD).astype(np.float32)
    std = rng.uniform(0.5, 60.0, FD).astype(np.float32)
    return win, mean, std


@pytest.mark.parametrize('norm', [False, True], ids=['raw', 'denorm'])
@pytest.mark.parametrize('n,overlap', [(1, 0), (1, 4), (3, 0), (3, 1), (3, 4)])
def test_track_blend_matches_float64(n, overlap, norm):
    import torch
    from a2m.inference import blend_track
    from a2m.normalization import denormalize
    win, mean, std = blend_inputs(n)
    d_win = torch.from_numpy(win).cuda()
    d_mean, d_std = (torch.from_numpy(mean).cuda(), torch.from_numpy(std).cuda()) if norm else (None, None)
    got = blend_track(d_win, overlap, d_mean, d_std).cpu().numpy()
    ref, cover = R.blend(win, overlap, mean if norm else None, std if norm else None)
    h = T - overlap
    assert got.shape == ref.shape == ((n - 1) * h + T, FD)
    single = denormalize(d_win, d_mean, d_std).cpu().numpy() if norm else win
    for f in np.flatnonzero(cover == 1):
        k = min(f // h, n - 1)
        assert np.array_equal(got[f], single[k, f - k * h]), f
    assert (cover == 2).sum() == (n - 1) * overlap
    if (cover == 2).any():
        ref32 = ref[cover == 2].astype(np.float32)
        ulps = np.abs(got[cover == 2].astype(np.float64) - ref[cover == 2]) / np.spacing(np.abs(ref32))
        print(f'n {n} overlap {overlap} norm {norm}: worst {ulps.max():.2f} ulp')
        assert ulps.max() <= 4


def test_track_blend_rejects_bad_arguments():
    import torch
    from a2m.inference import blend_track
    win = torch.zeros(2, T, FD, device='cuda')
    with pytest.raises(ValueError):
        blend_track(win, T // 2 + 1)
    with pytest.raises(ValueError):
        blend_track(win, 2, pose_mean=torch.zeros(FD, device='cuda'))
    assert tuple(blend_track(win[:0], 2).shape) == (0, FD)


# ------------------------------------------------------------------------------ generate_track
@pytest.fixture(scope='module')
def generator(g_state):
    import torch
    from a2m.real_motion_model import SelfAttention_G
    g = SelfAttention_G(p=0.0)
    g.load_state_dict(g_state, strict=False)
    return g.to('cuda').eval()


def test_generate_track_on_a_12_second_wave(generator, tmp_path):
    import torch
    from a2m import video as V
    from oracle import synth
    from a2m import inference as I
    from a2m.pats_audio import num_frames
    sr = 45600
    wave = torch.from_numpy(synth.speech_like(1, 12 * sr, seed=11)[0]).cuda()
    rng = np.random.default_rng(5)
    mean = torch.from_numpy(rng.uniform(-50, 50, 104).astype(np.float32)).cuda()
    std = torch.from_numpy(rng.uniform(1, 40, 104).astype(np.float32)).cuda()
    nf = num_frames(wave.shape[0], 2048, 512, True)
    for overlap in (0, 16):
        starts, window, interval, Tw = I.track_starts(nf, overlap)
        n, h = len(starts), 64 - overlap
        assert Tw == 64 and n >= 2 and starts[-1] + window <= nf < starts[-1] + h * interval + window
        track = I.generate_track(generator, wave, sr, overlap=overlap, pose_mean=mean, pose_std=std)
        assert tuple(track.shape) == ((n - 1) * h + 64, 104)
        windows = I.generate_from_wave(generator, wave, sr, starts=starts, pose_mean=mean, pose_std=std)
        if overlap == 0:
            assert torch.equal(track, windows.reshape(-1, 104))
        for k in range(n):
            lo = overlap if k > 0 else 0
            hi = 64 - overlap if k < n - 1 else 64
            assert torch.equal(track[k * h + lo:k * h + hi], windows[k, lo:hi]), (overlap, k)
    with pytest.raises(ValueError):
        I.generate_track(generator, wave[:2 * sr], sr)
    # the generated track, drawn: [F, 104] -> [F, 2, 52] -> a file the parser reads back
    frames = I.planar_frames(track[None])[0]
    fn = str(tmp_path / 'track.y4m')
    kw = dict(img_size=(400, 300), scale=0.25, line_width=8.0)
    assert V.save_pose_video(frames + 150.0, fn, chunk=50, **kw) == len(track)
    hdr, planes = R.parse_y4m(fn)
    assert (hdr['W'], hdr['H']) == ('100', '75') and planes.shape == (len(track), 3, 75, 100)
    assert (planes[:, 0] != 235).any()


# ------------------------------------------------------------------------------ the video file
def test_save_side_by_side_video(tmp_path):
    import torch
    from a2m import video as V
    canvas = (97, 41)
    k1 = render_case('generic', canvas)['kp'][:, 0]
    k1 = np.concatenate([k1, render_case('crossing', canvas)['kp'][:2, 0]])          # 5 frames
    k2 = np.concatenate([render_case('zero_length', canvas)['kp'][:, 0],
                         render_case('skeleton', canvas)['kp'][:, 0],
                         render_case('hairline', canvas)['kp'][:1, 0]])              # 7 frames
    fn = str(tmp_path / 'pair.y4m')
    kw = dict(img_size=canvas, scale=1.0, line_width=3.0)
    frames = V.save_side_by_side_video(str(tmp_path / 'unused'), k1, k2, fn, chunk=3, **kw)
    hdr, planes = R.parse_y4m(fn)
    with open(fn, 'rb') as f:
        assert f.readline() == b'YUV4MPEG2 W97 H41 F30000:2002 Ip A1:1 C444\n'
    assert frames == 7 and planes.shape == (7, 3, 41, 97)
    assert not (tmp_path / 'unused').exists()
    ycc, bg = V.rgb_to_ycbcr(np.array(V.REFERENCE_COLORS)), V.rgb_to_ycbcr(np.array((255, 255, 255)))
    direct = dict(colors=ycc, canvas=canvas, scale=1.0, line_width=3.0, background=bg)
    alone = V.render_poses(k2[:2], **direct)
    pair = V.render_poses(np.stack([k1, k2[2:]], 1), **direct)
    assert np.array_equal(planes[:2], alone) and np.array_equal(planes[2:], pair)
    assert (planes[:, 0] == 235).any() and (planes[:, 1:] == 128).any()       # white in limited range

    fn1 = str(tmp_path / 'single.y4m')
    assert V.save_pose_video(torch.from_numpy(k1).cuda(), fn1, **kw) == 5
    assert np.array_equal(R.parse_y4m(fn1)[1], V.render_poses(k1, **direct))


def test_draw_functions_write_ppm(tmp_path):
    from a2m import video as V
    case = render_case('two_poses', CANVASES[0])
    a, b = case['kp'][0, 0], case['kp'][0, 1]
    fn = tmp_path / 'pair.ppm'
    frame = V.draw_side_by_side_poses(None, a, b, output=str(fn), title='ignored', img_size=CANVASES[0],
                                      scale=1.0, line_width=3.0)
    assert np.array_equal(frame, V.render_poses(case['kp'][:1], canvas=CANVASES[0], scale=1.0,
                                                line_width=3.0)[0])
    raw = fn.read_bytes()
    assert raw.startswith(b'P6\n96 40\n255\n')
    assert np.array_equal(np.frombuffer(raw[len(b'P6\n96 40\n255\n'):], np.uint8).reshape(40, 96, 3),
                          frame.transpose(1, 2, 0))
    one = V.draw_pose(None, a, img_width=96, img_height=40, line_width=3.0)
    assert np.array_equal(one, V.render_poses(a[None], canvas=CANVASES[0], scale=1.0, line_width=3.0)[0])
    with pytest.raises(NotImplementedError):
        V.draw_pose('frame.jpg', a)
