"""csrc/jpeg.hip on the GPU against tests/jpeg_ref.py, byte for byte: a2m_jpeg_encode_u8 through
a2m.jpeg, then the surface above it -- write_jpeg, the Motion-JPEG AVI writers with sound, and
generate_video.  The encoder is integer arithmetic throughout, so there is no tolerance: every
file equals the restatement's (tests/test_jpeg_ref_cpu.py pins the restatement against PIL).
"""
import functools
import struct

import numpy as np
import pytest

import jpeg_ref as J

pytestmark = pytest.mark.gpu

CASE_IDS = [J.case_id(c) for c in J.CASES]
LINES = CASE_IDS.index('lines-200x64x2-q3')


@functools.lru_cache(maxsize=None)
def _rendered():
    """The 'lines' case on the GPU: two frames from render_poses with the full-range palette, and
    the restatement's files for them (computed once, read-only)."""
    from a2m import video as V
    W, H, N = J.CASES[LINES][1]
    rng = np.random.default_rng(31)
    kp = np.empty((N, 2, 52), np.float32)
    kp[:, 0], kp[:, 1] = rng.uniform(4, W - 4, (N, 52)), rng.uniform(4, H - 4, (N, 52))
    frames = V.render_poses(kp, colors=V.rgb_to_ycbcr_full(np.array(V.REFERENCE_COLORS)), canvas=(W, H),
                            scale=1.0, line_width=2.0,
                            background=V.rgb_to_ycbcr_full(np.array((255, 255, 255))))
    frames.setflags(write=False)
    return frames, tuple(J.encode(fr, J.CASES[LINES][2]) for fr in frames)


def _case(index):
    return _rendered() if index == LINES else J.encoded_case(index)


@pytest.mark.parametrize('index', range(len(J.CASES)), ids=CASE_IDS)
def test_files_equal_the_restatement(index):
    import torch
    from a2m import jpeg as A
    content, (W, H, N), qt = J.CASES[index]
    frames, files = _case(index)
    assert frames.shape == (N, 3, H, W)
    if index == LINES:
        assert (frames[:, 0] != 255).any() and (frames[:, 0] == 255).any()        # lines on white
    got = A.encode_jpeg(torch.from_numpy(np.array(frames)).cuda(), qtables=qt)
    assert len(got) == N
    for n in range(N):
        assert len(got[n]) == len(files[n]), (n, len(got[n]), len(files[n]))
        assert got[n] == files[n], n


def test_a_frame_of_the_default_canvas():
    """1500 x 500, what save_pose_avi encodes by default: 188 MCUs (564 blocks) in an interval and
    63 intervals, a pose drawn by the rasteriser."""
    import torch
    from a2m import jpeg as A
    from a2m import video as V
    rng = np.random.default_rng(12)
    kp = np.stack([rng.uniform(1000, 2000, 52), rng.uniform(100, 900, 52)]).astype(np.float32)[None]
    frames = V.render_poses(torch.from_numpy(kp).cuda(), colors=V.rgb_to_ycbcr_full(np.array(V.REFERENCE_COLORS)),
                            background=V.rgb_to_ycbcr_full(np.array((255, 255, 255))))
    assert tuple(frames.shape) == (1, 3, 500, 1500)
    got = A.encode_jpeg(frames, quality=90)[0]
    want = J.encode(frames[0].cpu().numpy(), J.quant_tables(90))
    assert len(got) == len(want) and got == want
    assert len(want) > 30000                                  # more than the 20.7 KB of a white frame


def test_quality_argument_and_empty_batch():
    import torch
    from a2m import jpeg as A
    frames, _ = J.encoded_case(CASE_IDS.index('noise-13x9x2-q16'))
    got = A.encode_jpeg(torch.from_numpy(np.array(frames)).cuda(), quality=75)
    assert got == [J.encode(fr, J.quant_tables(75)) for fr in frames]
    assert A.encode_jpeg(torch.empty(0, 3, 9, 13, dtype=torch.uint8, device='cuda')) == []
    buf, off = A.encode_scans(torch.empty(0, 3, 9, 13, dtype=torch.uint8, device='cuda'), J.quant_tables(75))
    assert len(buf) == 0 and off.tolist() == [0]
    with pytest.raises(ValueError):
        A.encode_jpeg(torch.zeros(1, 3, 9, 13, device='cuda'))                    # not uint8
    with pytest.raises(ValueError):
        A.encode_jpeg(torch.zeros(1, 3, 9, 13, dtype=torch.uint8, device='cuda'), qtables=np.zeros((2, 64), int))


def test_small_capacity_reports_the_size_and_spares_the_guard():
    import torch
    from a2m import jpeg as A
    index = CASE_IDS.index('noise-16x8x3-q1')
    _, (W, H, N), qt = J.CASES[index]
    frames, files = J.encoded_case(index)
    hdr = len(J.header(W, H, qt))
    scans = [f[hdr:-2] for f in files]
    whole = b''.join(scans)
    dev = torch.from_numpy(np.array(frames)).cuda()
    ws = torch.empty(A.workspace_bytes(N, W, H), dtype=torch.uint8, device='cuda')
    offsets = torch.empty(N + 1, dtype=torch.int64, device='cuda')
    for cap in (0, 1, len(scans[0]) + 3, len(whole) - 1, len(whole)):
        store = torch.full((cap + 64,), 0xA5, dtype=torch.uint8, device='cuda')
        A.encode_scans_into(dev, qt, store[:cap], offsets, ws)
        assert offsets.cpu().tolist() == np.concatenate([[0], np.cumsum([len(s) for s in scans])]).tolist()
        host = store.cpu().numpy()
        assert (host[cap:] == 0xA5).all(), cap
        assert host[:cap].tobytes() == whole[:cap], cap
    buf, off = A.encode_scans(dev, qt, capacity=10)                               # the retry
    assert buf.tobytes() == whole and int(off[N]) == len(whole)
    with pytest.raises(ValueError):
        A.encode_scans_into(dev, qt, store[:4], offsets, ws[:-1])                 # workspace too small


def test_graph_replay_of_render_and_encode():
    import torch
    from a2m import jpeg as A
    from a2m import video as V
    W, H = 16, 8
    qt = J.quant_tables(90)
    rng = np.random.default_rng(9)
    kps = [torch.from_numpy(rng.uniform(1, 15, (1, 2, 52)).astype(np.float32) * [[[1.0], [0.5]]]).float().cuda()
           for _ in range(2)]
    kw = dict(colors=V.rgb_to_ycbcr_full(np.array(V.REFERENCE_COLORS)), canvas=(W, H), scale=1.0,
              line_width=1.5, background=V.rgb_to_ycbcr_full(np.array((255, 255, 255))))
    eager = [A.encode_jpeg(V.render_poses(kp, **kw), qtables=qt)[0] for kp in kps]
    assert eager[0] != eager[1]
    hdr = len(J.header(W, H, qt))
    kp = kps[0].clone()
    frames = torch.zeros(1, 3, H, W, dtype=torch.uint8, device='cuda')
    out = torch.zeros(4096, dtype=torch.uint8, device='cuda')
    offsets = torch.zeros(2, dtype=torch.int64, device='cuda')
    ws = torch.empty(A.workspace_bytes(1, W, H), dtype=torch.uint8, device='cuda')
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        V.render_poses(kp, out=frames, **kw)
        A.encode_scans_into(frames, qt, out, offsets, ws)
    for k in (0, 1, 0):
        kp.copy_(kps[k])
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        lo, hi = offsets.cpu().tolist()
        assert lo == 0 and out[:hi].cpu().numpy().tobytes() == eager[k][hdr:-2], k


def test_write_jpeg(tmp_path):
    import torch
    from a2m import jpeg as A
    from a2m import video as V
    rng = np.random.default_rng(4)
    pose = np.stack([rng.uniform(3, 93, 52), rng.uniform(3, 37, 52)]).astype(np.float32)
    frame = V.draw_pose(None, pose, img_width=96, img_height=40, line_width=3.0)     # RGB [3, 40, 96]
    fn = tmp_path / 'pose.jpg'
    V.write_jpeg(str(fn), frame, quality=80)
    ycc = np.ascontiguousarray(V.rgb_to_ycbcr_full(frame.transpose(1, 2, 0)).transpose(2, 0, 1))
    data = fn.read_bytes()
    assert data == A.encode_jpeg(torch.from_numpy(ycc)[None].cuda(), quality=80)[0]
    assert data == J.encode(ycc, J.quant_tables(80))
    assert V.rgb_to_ycbcr_full(np.array([(255, 255, 255), (255, 0, 0), (0, 0, 0)])).tolist() == \
        [[255, 128, 128], [76, 85, 255], [0, 128, 128]]


# ------------------------------------------------------------------------------ the AVI file
def parse_avi(path):
    """A reader of this test's own: -> dict(data, lists {kind: (pos of 'LIST', size)}, chunks
    {fourcc: [(pos of the chunk header, payload)]}) over the whole RIFF tree."""
    data = open(path, 'rb').read()
    assert data[:4] == b'RIFF' and data[8:12] == b'AVI '
    assert struct.unpack('<I', data[4:8])[0] == len(data) - 8
    lists, chunks = {}, {}

    def walk(lo, hi):
        while lo < hi:
            cc, size = data[lo:lo + 4], struct.unpack('<I', data[lo + 4:lo + 8])[0]
            assert lo + 8 + size <= hi, (cc, lo, size, hi)
            if cc == b'LIST':
                lists.setdefault(data[lo + 8:lo + 12], []).append((lo, size))
                walk(lo + 12, lo + 8 + size)
            else:
                chunks.setdefault(cc, []).append((lo, data[lo + 8:lo + 8 + size]))
            lo += 8 + size + (size & 1)
        assert lo == hi, 'chunks are padded to even length and fill their list exactly'

    walk(12, len(data))
    return dict(data=data, lists=lists, chunks=chunks)


def test_save_side_by_side_avi(tmp_path):
    import torch
    from a2m import jpeg as A
    from a2m import video as V
    from test_gpu_render import render_case
    canvas = (97, 41)
    k1 = render_case('generic', canvas)['kp'][:, 0]
    k1 = np.concatenate([k1, render_case('crossing', canvas)['kp'][:2, 0]])          # 5 frames
    k2 = np.concatenate([render_case('zero_length', canvas)['kp'][:, 0],
                         render_case('skeleton', canvas)['kp'][:, 0],
                         render_case('hairline', canvas)['kp'][:1, 0]])              # 7 frames
    sr = 8000
    wave = 0.8 * np.sin(2 * np.pi * 440 * np.arange(sr // 2) / sr)                   # 0.5 s
    wave[:3] = (1.5, -1.5, 0.25)                                                     # clipped
    fn = str(tmp_path / 'pair.avi')
    kw = dict(img_size=canvas, scale=1.0, line_width=3.0)
    assert V.save_side_by_side_avi(k1, k2, fn, wave=wave, sr=sr, quality=85, chunk=3, **kw) == 7
    avi = parse_avi(fn)
    data, chunks = avi['data'], avi['chunks']
    assert len(chunks[b'00dc']) == 7 and len(chunks[b'01wb']) == 7
    assert set(avi['lists']) == {b'hdrl', b'strl', b'movi'} and len(avi['lists'][b'strl']) == 2
    avih = struct.unpack('<14I', chunks[b'avih'][0][1])
    assert avih[0] == 66733 and avih[4] == 7 and avih[6] == 2 and avih[8:10] == (97, 41)
    vids, auds = (struct.unpack('<4s4sIHHIIIIIIII4H', c[1]) for c in chunks[b'strh'])
    assert vids[:2] == (b'vids', b'MJPG') and (vids[7], vids[6]) == (30000, 2002) and vids[9] == 7
    assert auds[0] == b'auds' and (auds[7], auds[6]) == (sr, 1) and auds[12] == 2
    assert struct.unpack('<IiiHH4s', chunks[b'strf'][0][1][:20]) == (40, 97, 41, 1, 24, b'MJPG')
    assert struct.unpack('<HHIIHH', chunks[b'strf'][1][1]) == (1, 1, sr, 2 * sr, 2, 16)
    # idx1: offsets from the 'movi' fourcc land on the chunk headers, in file order
    movi = avi['lists'][b'movi'][0][0] + 8
    idx = chunks[b'idx1'][0][1]
    entries = [struct.unpack('<4sIII', idx[16 * k:16 * k + 16]) for k in range(len(idx) // 16)]
    assert [e[0] for e in entries] == [b'00dc', b'01wb'] * 7
    ordered = sorted(chunks[b'00dc'] + chunks[b'01wb'])
    for (cc, flags, off, size), (pos, payload) in zip(entries, ordered):
        assert movi + off == pos and data[pos:pos + 4] == cc and size == len(payload) and flags == 0x10
    assert len(data) == chunks[b'idx1'][0][0] + 8 + len(idx)                         # idx1 ends the file
    # the pictures: the first two frames show keypoints2 alone
    ycc, bg = V.rgb_to_ycbcr_full(np.array(V.REFERENCE_COLORS)), V.rgb_to_ycbcr_full(np.array((255, 255, 255)))
    direct = dict(colors=ycc, canvas=canvas, scale=1.0, line_width=3.0, background=bg)
    alone = V.render_poses(torch.from_numpy(k2[:2]).cuda(), **direct)
    pair = V.render_poses(torch.from_numpy(np.stack([k1, k2[2:]], 1)).cuda(), **direct)
    files = A.encode_jpeg(torch.cat([alone, pair]), quality=85)
    assert [p for _, p in chunks[b'00dc']] == files
    assert files[0] == J.encode(alone[0].cpu().numpy(), J.quant_tables(85))
    # the sound: the quantised wave cut to 7 frames, split with no sample lost or doubled
    pcm = np.rint(np.clip(wave, -1, 1) * 32767).astype('<i2')
    assert pcm[0] == 32767 and pcm[1] == -32767
    total = 7 * sr * 2002 // 30000
    assert total < len(pcm)
    assert b''.join(p for _, p in chunks[b'01wb']) == pcm[:total].tobytes()
    assert [len(p) // 2 for _, p in chunks[b'01wb']] == \
        [(i + 1) * sr * 2002 // 30000 - i * sr * 2002 // 30000 for i in range(7)]
    assert auds[9] == total

    fn1 = str(tmp_path / 'single.avi')
    assert V.save_pose_avi(torch.from_numpy(k1).cuda(), fn1, quality=85, **kw) == 5
    single = parse_avi(fn1)
    assert b'01wb' not in single['chunks'] and len(single['lists'][b'strl']) == 1
    assert [p for _, p in single['chunks'][b'00dc']] == \
        A.encode_jpeg(V.render_poses(torch.from_numpy(k1).cuda(), **direct), quality=85)
    with pytest.raises(ValueError):
        V.save_pose_avi(k1, str(tmp_path / 'single.y4m'), **kw)
    with pytest.raises(ValueError):
        V.save_pose_avi(k1, fn1, wave=wave, **kw)                                    # wave without sr


@pytest.fixture(scope='module')
def generator(g_state):
    from a2m.real_motion_model import SelfAttention_G
    g = SelfAttention_G(p=0.0)
    g.load_state_dict(g_state, strict=False)
    return g.to('cuda').eval()


def test_generate_video_on_a_12_second_wave(generator, tmp_path):
    import torch
    from oracle import synth
    from a2m import inference as I
    sr = 45600
    wave = torch.from_numpy(synth.speech_like(1, 12 * sr, seed=11)[0]).cuda()
    rng = np.random.default_rng(5)
    mean = torch.from_numpy(rng.uniform(100, 200, 104).astype(np.float32)).cuda()
    std = torch.from_numpy(rng.uniform(1, 40, 104).astype(np.float32)).cuda()
    track = I.generate_track(generator, wave, sr, overlap=16, pose_mean=mean, pose_std=std)
    fn = str(tmp_path / 'track.avi')
    frames = I.generate_video(generator, wave, sr, fn, overlap=16, pose_mean=mean, pose_std=std,
                              img_size=(400, 300), scale=0.25, line_width=8.0, chunk=50)
    assert frames == len(track)
    avi = parse_avi(fn)
    assert len(avi['chunks'][b'00dc']) == frames and len(avi['chunks'][b'01wb']) == frames
    first = J.decode(avi['chunks'][b'00dc'][0][1])
    assert (first['W'], first['H']) == (100, 75)
    assert any((J.decode(p)['coef'][..., 1:] != 0).any() for _, p in avi['chunks'][b'00dc'][:3])   # lines drawn
    sound = np.frombuffer(b''.join(p for _, p in avi['chunks'][b'01wb']), '<i2')
    assert len(sound) == frames * sr * 2002 // 30000
    want = np.rint(np.clip(wave.cpu().numpy().astype(np.float64), -1, 1) * 32767).astype('<i2')
    assert np.array_equal(sound, want[:len(sound)])
    with pytest.raises(ValueError):
        I.generate_video(generator, wave, sr, str(tmp_path / 'track.mp4'))
