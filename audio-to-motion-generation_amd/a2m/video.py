"""Pose tracks to video frames on the device: the plotting surface of
generate_motion_video.py:23-200 over the a2m_render_poses_u8 rasteriser (csrc/render.hip).

  render_poses(keypoints, ...)                    [N,2,K] / [N,P,2,K] -> uint8 [N,3,H,W]
  draw_pose(img, keypoints, ...)                  :103-136  one frame, one pose
  draw_side_by_side_poses(img, kp1, kp2, ...)     :139-164  one frame, two poses on one canvas
  save_side_by_side_video(tmp, kp1, kp2, fn, ...) :167-190  a YUV4MPEG2 file (no JPEGs, no ffmpeg)
  save_pose_video(keypoints, fn, ...)             the same for a single track
  save_side_by_side_avi(kp1, kp2, fn, wave, sr)   the same as Motion-JPEG AVI with sound: frames
  save_pose_avi(keypoints, fn, wave, sr, ...)     compressed on the device (a2m.jpeg, a2m.avi)
  write_jpeg(path, frame, quality)                :174-185  one RGB frame as a .jpg file
  save_video_from_audio_video(wav, avi, out)      :203-207  a .wav under the picture of an .avi

What is drawn is the pixel function documented in include/a2m.h: round-capped polylines with a
one-pixel linear edge.  matplotlib, PIL and ffmpeg are not used; parity with matplotlib's Agg
output is UNPINNED (its caps and anti-aliasing differ, and the library is absent where this was
built): the float64 restatement in tests/render_ref.py is the only pin.  No text is drawn, so
`title` arguments are accepted and ignored, and there is no image decoder, so `img` must be None.

REFERENCE_POLYLINES are the reference's draw groups in its draw order: the head lines (purple),
right body (gray), left body (blue), five left-hand fingers (red), five right-hand fingers
(yellow).  The reference's right-hand lists are [31, 29+4i .. 32+4i] as written (they start two
keypoints before the hand's first finger joint); we draw what it draws.  SKELETON_POLYLINES is the
real topology instead: one two-point bone per joint of a2m.skeleton.Skeleton2D().parents.
"""
import numpy as np
import torch

from . import avi, jpeg
from . import functional as F
from ._native import check, lib
from .avi import save_video_from_audio_video  # noqa: F401  (generate_motion_video.py:203-207)
from .skeleton import Skeleton2D

PURPLE, GRAY, BLUE, RED, YELLOW = (128, 0, 128), (128, 128, 128), (0, 0, 255), (255, 0, 0), (255, 255, 0)

REFERENCE_POLYLINES = (
    (7, 8), (7, 9),
    (1, 2, 3, 31),
    (4, 5, 6, 10),
    (10, 11, 12, 13, 14), (10, 15, 16, 17, 18), (10, 19, 20, 21, 22), (10, 23, 24, 25, 26),
    (10, 27, 28, 29, 30),
    (31, 29, 30, 31, 32), (31, 33, 34, 35, 36), (31, 37, 38, 39, 40), (31, 41, 42, 43, 44),
    (31, 45, 46, 47, 48),
)
REFERENCE_COLORS = (PURPLE, PURPLE, GRAY, BLUE) + (RED,) * 5 + (YELLOW,) * 5

SKELETON_POLYLINES = tuple((p, j) for j, p in enumerate(Skeleton2D().parents) if p >= 0)
SKELETON_COLORS = tuple(PURPLE if j in (7, 8, 9) else GRAY if j < 4 else BLUE if j < 7 else
                        RED if j < 31 else YELLOW for _, j in SKELETON_POLYLINES)

# the reference's 1.5 pt line at dpi 400 on its 2400-pixel-wide axes showing 3000 data units
REFERENCE_LINE_WIDTH = 1.5 * 400 / 72 / 0.8
FPS = (30000, 2002)   # the reference's ffmpeg input rate, -r 30000/2002


def _colors(polylines, colors):
    """colors=None: the reference's palette for its draw groups, the same hues per limb for
    SKELETON_POLYLINES, gray for any other list."""
    if colors is not None:
        return colors
    lines = tuple(tuple(line) for line in polylines)
    return REFERENCE_COLORS if lines == REFERENCE_POLYLINES else \
        SKELETON_COLORS if lines == SKELETON_POLYLINES else (GRAY,) * len(lines)


def _y4m_name(output_fn):
    if not str(output_fn).endswith('.y4m'):
        raise ValueError(f'the video is written as YUV4MPEG2: output_fn must end in .y4m, got {output_fn!r}')


def _tables(polylines, colors, K):
    """Validated (poly_idx, poly_off, poly_rgb) numpy arrays for the C entry point."""
    lines = [tuple(int(i) for i in line) for line in polylines]
    colors = _colors(lines, colors)
    if len(colors) != len(lines):
        raise ValueError(f'{len(lines)} polylines but {len(colors)} colors')
    for l, line in enumerate(lines):
        if len(line) < 2:
            raise ValueError(f'polyline {l} has {len(line)} point(s); a line needs at least 2')
        for i in line:
            if not 0 <= i < K:
                raise ValueError(f'polyline {l}: keypoint index {i} outside [0, {K})')
    idx = np.array([i for line in lines for i in line], np.int32)
    off = np.concatenate([[0], np.cumsum([len(line) for line in lines])]).astype(np.int32)
    rgb = np.asarray(colors, np.int64).reshape(-1, 3)
    if rgb.size and (rgb.min() < 0 or rgb.max() > 255):
        raise ValueError('colors are bytes (0..255)')
    return idx, off, np.ascontiguousarray(rgb.astype(np.uint8))


def _geometry(P, canvas, scale, line_width, offsets):
    """-> (W, H, xform float32 [P, 4], half_width_px)."""
    W, H = int(round(canvas[0] * scale)), int(round(canvas[1] * scale))
    if W < 1 or H < 1:
        raise ValueError(f'canvas {tuple(canvas)} at scale {scale} has no pixels')
    off = np.zeros((P, 2), np.float64) if offsets is None else np.asarray(offsets, np.float64)
    if off.shape != (P, 2):
        raise ValueError(f'offsets must be [{P}, 2] (one x, y shift per pose), got {off.shape}')
    lw = REFERENCE_LINE_WIDTH if line_width is None else float(line_width)
    if not (np.isfinite(lw) and lw >= 0):
        raise ValueError(f'line_width must be finite and >= 0, got {line_width!r}')
    xf = np.empty((P, 4), np.float32)
    xf[:, 0] = xf[:, 2] = scale            # ylim (H, 0): y points down, as pixel rows do
    xf[:, 1], xf[:, 3] = scale * off[:, 0], scale * off[:, 1]
    return W, H, xf, 0.5 * lw * scale


_xforms = {}


def _shape4(shape):
    if len(shape) == 3 and shape[1] == 2:
        return (shape[0], 1, 2, shape[2])
    if len(shape) == 4 and shape[2] == 2:
        return tuple(shape)
    raise ValueError(f'keypoints must be [N, 2, K] or [N, P, 2, K], got {tuple(shape)}')


def render_poses(keypoints, polylines=REFERENCE_POLYLINES, colors=None,
                 canvas=(3000, 1000), scale=0.5, line_width=None, offsets=None,
                 background=(255, 255, 255), out=None):
    """keypoints [N, 2, K] or [N, P, 2, K] (x row, y row; P poses drawn over each other in order)
    -> uint8 [N, 3, H, W] planar frames.  numpy in -> numpy out; device tensors in -> device out.

    canvas = (width, height) of the reference's data window (xlim (0, width), ylim (height, 0));
    scale maps data units to pixels, so the frame is round(width*scale) x round(height*scale);
    line_width is in data units (default: the reference's 1.5 pt line, about 10.42 units);
    offsets [P, 2] shifts pose p by (x, y) data units; out: a contiguous uint8 device tensor
    [N, 3, H, W] written in place.  The call is one stream-ordered launch and can be captured
    in a HIP graph once the same geometry has been rendered before (its [P, 4] transform is
    uploaded on first use)."""
    as_numpy = not torch.is_tensor(keypoints)
    N, P, _, K = _shape4(np.shape(keypoints) if as_numpy else keypoints.shape)
    idx, off, rgb = _tables(polylines, colors, K)
    W, H, xf, hw = _geometry(P, canvas, scale, line_width, offsets)
    bg = np.asarray(background, np.int64).reshape(-1)
    if bg.shape != (3,) or bg.min() < 0 or bg.max() > 255:
        raise ValueError('background is three bytes')
    bg = bg.astype(np.uint8)
    kp = torch.as_tensor(np.asarray(keypoints, np.float32)).cuda() if as_numpy else keypoints
    F._check_dev(kp)
    kp = kp.contiguous()
    if out is None:
        out = torch.empty(N, 3, H, W, dtype=torch.uint8, device=kp.device)
    elif not (torch.is_tensor(out) and out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous()
              and tuple(out.shape) == (N, 3, H, W)):
        raise ValueError(f'out must be a contiguous uint8 device tensor [{N}, 3, {H}, {W}]')
    key = (xf.tobytes(), str(kp.device))
    if key not in _xforms:          # a few small tables; a render inside a graph capture needs a hit
        _xforms[key] = torch.from_numpy(xf).to(kp.device)
    xf_d = _xforms[key]
    check(lib.a2m_render_poses_u8(F._p(kp), N, P, K, idx.ctypes.data, off.ctypes.data, rgb.ctypes.data,
                                  len(off) - 1, F._p(xf_d), hw, bg.ctypes.data, W, H, F._p(out),
                                  F._stream()), value_error=True)
    return out.cpu().numpy() if as_numpy else out


def write_ppm(path, frame):
    """frame uint8 [3, H, W] (numpy or tensor) -> binary PPM (P6)."""
    fr = frame.cpu().numpy() if torch.is_tensor(frame) else np.asarray(frame)
    _, H, W = fr.shape
    with open(path, 'wb') as f:
        f.write(b'P6\n%d %d\n255\n' % (W, H))
        f.write(np.ascontiguousarray(fr.transpose(1, 2, 0)).tobytes())


def _one(keypoints):
    as_numpy = not torch.is_tensor(keypoints)
    kp = np.asarray(keypoints, np.float32) if as_numpy else keypoints
    if kp.ndim != 2 or kp.shape[0] != 2:
        raise ValueError(f'one pose is [2, K], got {tuple(kp.shape)}')
    return kp


def _no_image(img):
    if img is not None:
        raise NotImplementedError('drawing over an image needs an image decoder, which a2m does not have; '
                                  'pass img=None')


def draw_pose(img, keypoints, img_width=1280, img_height=720, output=None, title=None, title_x=1,
              line_width=None, scale=1.0, polylines=REFERENCE_POLYLINES, colors=None):
    """generate_motion_video.draw_pose: keypoints [2, K] on a white img_width x img_height canvas
    -> uint8 [3, H, W].  img must be None; title / title_x are accepted and ignored (no text is
    drawn); output: path of a binary PPM to write."""
    _no_image(img)
    frame = render_poses(_one(keypoints)[None], polylines, colors, (img_width, img_height), scale,
                         line_width)[0]
    if output:
        write_ppm(output, frame)
    return frame


def draw_side_by_side_poses(img, keypoints1, keypoints2, output=None, show=False, title=None,
                            img_size=(3000, 1000), line_width=None, scale=0.5,
                            polylines=REFERENCE_POLYLINES, colors=None):
    """generate_motion_video.draw_side_by_side_poses: both poses ([2, K] each) on one img_size
    canvas, keypoints1 first -> uint8 [3, H, W].  img must be None; show and title are accepted
    and ignored (no text is drawn); output: path of a binary PPM to write."""
    _no_image(img)
    k1, k2 = _one(keypoints1), _one(keypoints2)
    pair = torch.stack([k1, k2]) if torch.is_tensor(k1) else np.stack([k1, k2])
    frame = render_poses(pair[None], polylines, colors, img_size, scale, line_width)[0]
    if output:
        write_ppm(output, frame)
    return frame


# ------------------------------------------------------------------------------ YUV4MPEG2
def rgb_to_ycbcr(rgb):
    """BT.601 limited-range YCbCr bytes of RGB bytes [..., 3]."""
    c = np.asarray(rgb, np.float64) / 255.0
    r, g, b = c[..., 0], c[..., 1], c[..., 2]
    y = 0.299 * r + 0.587 * g + 0.114 * b
    ycc = np.stack([16 + 219 * y, 128 + 224 * (b - y) / 1.772, 128 + 224 * (r - y) / 1.402], -1)
    return np.clip(np.floor(ycc + 0.5), 0, 255).astype(np.uint8)


class Y4MWriter:
    """A C444 YUV4MPEG2 stream: write(frames) appends uint8 [n, 3, H, W] (Y, Cb, Cr planes)."""

    def __init__(self, path, W, H, fps=FPS):
        _y4m_name(path)
        self.W, self.H, self.frames = int(W), int(H), 0
        self.f = open(path, 'wb')
        self.f.write(b'YUV4MPEG2 W%d H%d F%d:%d Ip A1:1 C444\n' % (self.W, self.H, fps[0], fps[1]))

    def write(self, frames):
        fr = np.ascontiguousarray(frames, np.uint8)
        if fr.ndim != 4 or fr.shape[1:] != (3, self.H, self.W):
            raise ValueError(f'frames must be [n, 3, {self.H}, {self.W}], got {fr.shape}')
        for one in fr:
            self.f.write(b'FRAME\n')
            self.f.write(one.data)
        self.frames += len(fr)

    def close(self):
        self.f.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


def write_y4m(path, frames, fps=FPS):
    """frames uint8 [n, 3, H, W], already Y, Cb, Cr planes -> a YUV4MPEG2 file."""
    fr = np.asarray(frames)
    if fr.ndim != 4 or fr.shape[1] != 3:
        raise ValueError(f'frames must be [n, 3, H, W], got {fr.shape}')
    with Y4MWriter(path, fr.shape[3], fr.shape[2], fps) as w:
        w.write(fr)


def _track(keypoints):
    """A track [n, 2, K] as a device tensor (n may be 0)."""
    if torch.is_tensor(keypoints):
        kp = keypoints.float()
    else:
        kp = torch.as_tensor(np.asarray(keypoints, np.float32))
    if kp.dim() != 3 or kp.shape[1] != 2:
        raise ValueError(f'a track is [n, 2, K], got {tuple(kp.shape)}')
    return kp.cuda()


def _write_video(output_fn, parts, polylines, colors, canvas, scale, line_width, background, fps, chunk):
    """parts: [frames, P, 2, K] device tensors rendered one after the other into one file.  The
    palette and the background go to YCbCr on the host; blending is affine, so the rasteriser
    then draws the Y, Cb and Cr planes directly."""
    if chunk < 1:
        raise ValueError('chunk must be >= 1')
    ycc = rgb_to_ycbcr(np.asarray(_colors(polylines, colors), np.uint8).reshape(-1, 3))
    bg = rgb_to_ycbcr(np.asarray(background, np.uint8))
    W, H = int(round(canvas[0] * scale)), int(round(canvas[1] * scale))
    pinned = torch.empty(chunk, 3, H, W, dtype=torch.uint8).pin_memory()
    dev = None
    with Y4MWriter(output_fn, W, H, fps) as w:
        for part in parts:
            for i in range(0, part.shape[0], chunk):
                kp = part[i:i + chunk]
                if dev is None or dev.shape[0] != kp.shape[0]:
                    dev = torch.empty(kp.shape[0], 3, H, W, dtype=torch.uint8, device=kp.device)
                render_poses(kp, polylines, ycc, canvas, scale, line_width, None, bg, out=dev)
                host = pinned[:kp.shape[0]]
                host.copy_(dev, non_blocking=True)
                torch.cuda.current_stream().synchronize()
                w.write(host.numpy())
        return w.frames


def save_side_by_side_video(temp_folder, keypoints1, keypoints2, output_fn, delete_tmp=True, fps=FPS,
                            chunk=64, polylines=REFERENCE_POLYLINES, colors=None,
                            img_size=(3000, 1000), scale=0.5, line_width=None,
                            background=(255, 255, 255)):
    """generate_motion_video.save_side_by_side_video: tracks [n, 2, K] drawn together frame by
    frame into a YUV4MPEG2 file (C444, BT.601 limited range) that ffmpeg, mpv and VLC read.  As
    in the reference, when keypoints2 is longer by `diff` frames, the first `diff` frames show
    keypoints2 alone.  `chunk` frames are rendered at a time and copied to the host through one
    pinned buffer.  temp_folder and delete_tmp are accepted for compatibility and not used (no
    image files are written).  Returns the number of frames."""
    _y4m_name(output_fn)
    k1, k2 = _track(keypoints1), _track(keypoints2)
    parts = []
    diff = k2.shape[0] - k1.shape[0]
    if diff > 0:
        parts.append(k2[:diff, None])
        k2 = k2[diff:]
    n = k1.shape[0]
    if k2.shape[0] < n:
        raise ValueError(f'keypoints2 has {k2.shape[0]} frames, fewer than keypoints1 ({n})')
    parts.append(torch.stack([k1, k2[:n]], 1))
    return _write_video(output_fn, parts, polylines, colors, img_size, scale, line_width, background, fps,
                        chunk)


def save_pose_video(keypoints, output_fn, fps=FPS, chunk=64, polylines=REFERENCE_POLYLINES,
                    colors=None, img_size=(3000, 1000), scale=0.5, line_width=None,
                    background=(255, 255, 255)):
    """One track [n, 2, K] -> a YUV4MPEG2 file, as save_side_by_side_video writes it."""
    _y4m_name(output_fn)
    return _write_video(output_fn, [_track(keypoints)[:, None]], polylines, colors, img_size, scale,
                        line_width, background, fps, chunk)


# ------------------------------------------------------------------------------ JPEG and AVI
def rgb_to_ycbcr_full(rgb):
    """JFIF (BT.601 full-range) YCbCr bytes of RGB bytes [..., 3]: the twin of rgb_to_ycbcr for
    the planes a JPEG holds."""
    c = np.asarray(rgb, np.float64)
    r, g, b = c[..., 0], c[..., 1], c[..., 2]
    y = 0.299 * r + 0.587 * g + 0.114 * b
    ycc = np.stack([y, 128 + (b - y) / 1.772, 128 + (r - y) / 1.402], -1)
    return np.clip(np.floor(ycc + 0.5), 0, 255).astype(np.uint8)


def write_jpeg(path, frame, quality=90):
    """An RGB frame uint8 [3, H, W] (numpy or tensor), as draw_pose returns it -> a baseline JPEG
    file (generate_motion_video.py:174-185 writes its %04d.jpg frames with matplotlib).  The
    pixels are converted to full-range YCbCr on the host; the encoder runs on the device."""
    fr = frame.cpu().numpy() if torch.is_tensor(frame) else np.asarray(frame)
    if fr.ndim != 3 or fr.shape[0] != 3 or fr.dtype != np.uint8:
        raise ValueError(f'frame must be uint8 [3, H, W], got {fr.dtype} {fr.shape}')
    ycc = np.ascontiguousarray(rgb_to_ycbcr_full(fr.transpose(1, 2, 0)).transpose(2, 0, 1))
    data = jpeg.encode_jpeg(torch.from_numpy(ycc)[None].cuda(), quality)[0]
    with open(path, 'wb') as f:
        f.write(data)


def _avi_name(output_fn):
    if not str(output_fn).endswith('.avi'):
        raise ValueError(f'the video is written as Motion-JPEG AVI: output_fn must end in .avi, got {output_fn!r}')


def _write_avi(output_fn, parts, wave, sr, quality, polylines, colors, canvas, scale, line_width, background,
               fps, chunk):
    """_write_video with the frames compressed on the device: each chunk is rendered with the
    full-range YCbCr palette into one device buffer and encoded there; the offsets, then only
    the compressed bytes (through one pinned buffer) cross to the host."""
    if chunk < 1:
        raise ValueError('chunk must be >= 1')
    if (wave is None) != (sr is None):
        raise ValueError('wave and sr come together')
    ycc = rgb_to_ycbcr_full(np.asarray(_colors(polylines, colors), np.uint8).reshape(-1, 3))
    bg = rgb_to_ycbcr_full(np.asarray(background, np.uint8))
    W, H = int(round(canvas[0] * scale)), int(round(canvas[1] * scale))
    qt = jpeg.quant_tables(quality)
    pcm = None if wave is None else avi.pcm16(wave)
    dev = None
    with avi.AVIWriter(output_fn, W, H, fps, audio_rate=sr) as w:
        header = jpeg.jpeg_header(W, H, qt)
        if pcm is not None:
            w.set_audio(pcm)
        for part in parts:
            for i in range(0, part.shape[0], chunk):
                kp = part[i:i + chunk]
                if dev is None or dev.shape[0] != kp.shape[0]:
                    dev = torch.empty(kp.shape[0], 3, H, W, dtype=torch.uint8, device=kp.device)
                render_poses(kp, polylines, ycc, canvas, scale, line_width, None, bg, out=dev)
                buf, off = jpeg.encode_scans(dev, qt)
                for n in range(kp.shape[0]):
                    w.write_frame(header, buf[off[n]:off[n + 1]].data, jpeg.EOI)
        return w.frames


def save_side_by_side_avi(keypoints1, keypoints2, output_fn, wave=None, sr=None, quality=90, fps=FPS,
                          chunk=64, polylines=REFERENCE_POLYLINES, colors=None, img_size=(3000, 1000),
                          scale=0.5, line_width=None, background=(255, 255, 255)):
    """save_side_by_side_video as a Motion-JPEG AVI, with `wave` (float [-1, 1], mono, at `sr`
    samples a second; numpy or tensor) as its sound track, cut to the picture's duration.  The
    frames are compressed on the device (a2m.jpeg); as in the reference, when keypoints2 is longer
    by `diff` frames, the first `diff` frames show keypoints2 alone.  Returns the number of
    frames."""
    _avi_name(output_fn)
    k1, k2 = _track(keypoints1), _track(keypoints2)
    parts = []
    diff = k2.shape[0] - k1.shape[0]
    if diff > 0:
        parts.append(k2[:diff, None])
        k2 = k2[diff:]
    n = k1.shape[0]
    if k2.shape[0] < n:
        raise ValueError(f'keypoints2 has {k2.shape[0]} frames, fewer than keypoints1 ({n})')
    parts.append(torch.stack([k1, k2[:n]], 1))
    return _write_avi(output_fn, parts, wave, sr, quality, polylines, colors, img_size, scale, line_width,
                      background, fps, chunk)


def save_pose_avi(keypoints, output_fn, wave=None, sr=None, quality=90, fps=FPS, chunk=64,
                  polylines=REFERENCE_POLYLINES, colors=None, img_size=(3000, 1000), scale=0.5,
                  line_width=None, background=(255, 255, 255)):
    """One track [n, 2, K] -> a Motion-JPEG AVI with sound, as save_side_by_side_avi writes it."""
    _avi_name(output_fn)
    return _write_avi(output_fn, [_track(keypoints)[:, None]], wave, sr, quality, polylines, colors,
                      img_size, scale, line_width, background, fps, chunk)
