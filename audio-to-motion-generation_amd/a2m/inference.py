"""Inference surface of generate_motion_video.py, on the device.

  load_generator(path)      :237-238  construct + load_state_dict (weights_only) + eval
  generate(g, audio, ...)   :247-260  generator(audio) on normalised audio features, then the
                                      normalised poses mapped back: pose * std + mean
  generate_from_wave(g, wave, sr, ...)  the same from a raw recording: PATS log_mel_512 windows
                                      (pats_audio.log_mel_512_windows) -> generate
  generate_track(g, wave, sr, overlap, ...)  a whole recording to ONE track [F, 104]: windows
                                      whose starts lie T - overlap pose frames apart, cross-faded
                                      and de-normalised in one pass (a2m_track_blend_f32)
  generate_video(g, wave, sr, fn, ...)  generate_track, drawn and written as a Motion-JPEG AVI
                                      with the recording as its sound track (a2m.video)
  planar_frames(pose)       :262-266  [B, T, 104] -> [B, T, 2, 52] (x row, y row) for plotting
  TrackStream(g, sr, ...) / VideoStream(g, sr, fn, ...)  generate_track / generate_video for audio
                                      that arrives in pieces: push(samples), close(); the pieces
                                      concatenate to the offline result bit for bit
                                      (TrackBlendStream: blend_track a few windows at a time)

  GraphedGenerator(g, ...)  HIP-graph replay of a fixed-shape eval forward (the serving loop
                            of :247-260 at a fixed batch): one graph per decoder branch, the
                            two branches on two streams joined by events

Plotting (:23-207) is a2m.video: a device rasteriser writing YUV4MPEG2 or, through the device JPEG
encoder of a2m.jpeg, Motion-JPEG AVI with sound; no matplotlib or ffmpeg.
"""
import torch

from . import functional as F
from .normalization import denormalize
from .real_motion_model import SelfAttention_G


def load_generator(path, device='cuda', **kwargs):
    g = SelfAttention_G(**kwargs)
    g.load_state_dict(torch.load(path, map_location='cpu', weights_only=True))
    return g.to(device).eval()


@torch.no_grad()
def generate(generator, audio, pose_mean=None, pose_std=None):
    """audio [B, T, 128] (device) -> poses [B, T, 104]; de-normalised when mean/std are given."""
    pose, _ = generator(audio)
    if pose_mean is not None:
        pose = denormalize(pose, pose_mean.to(pose.device), pose_std.to(pose.device))
    return pose


@torch.no_grad()
def generate_from_wave(generator, wave, sr, starts=None, time=4.3, fs_new=15, audio_mean=None,
                       audio_std=None, pose_mean=None, pose_std=None, resample_to=None,
                       res_type='kaiser_best', **mel_kwargs):
    """A recording to poses in one call: wave [S] (device) -> audio/log_mel_512 windows as the
    PATS loader cuts them (windowing.window_index: `time` seconds at 89 feature frames/s read
    every round(89 / fs_new)-th frame, i.e. 382 / 6 -> T = 64; only those frames are computed),
    standardised with audio_mean / audio_std when given -> generator -> poses [n, T, 104],
    de-normalised when pose_mean / pose_std are given.  `starts` (feature-frame index of each
    window) defaults to the loader's non-overlapping windows; mel_kwargs go to
    pats_audio.log_mel_512_windows (eps, pad_mode).  The windows assume the rate the PATS features
    were made at (89 frames/s x hop 512); a recording at another rate is brought there on the
    device with resample_to=<that rate> (pats_audio.resample, filter `res_type`), and everything
    downstream then takes resample_to as the rate.  None: the wave is used as it is."""
    from .pats_audio import log_mel_512_windows, num_frames, resample
    from .windowing import window_index
    if resample_to is not None:
        wave, sr = resample(wave, sr, resample_to, res_type), resample_to
    auto, window, interval = window_index(num_frames(wave.shape[-1], 2048, 512, True),
                                          'audio/log_mel_512', fs_new, time)
    audio = log_mel_512_windows(wave, sr, auto if starts is None else starts, window, interval,
                                audio_mean, audio_std, **mel_kwargs)
    return generate(generator, audio, pose_mean, pose_std)


def blend_track(windows, overlap, pose_mean=None, pose_std=None, out=None):
    """windows [n, T, Fd] (device) whose starts lie T - overlap frames apart -> one track
    [(n-1)(T-overlap) + T, Fd]: linear cross-fade over each overlap (weights (j + 0.5)/overlap and
    its complement), then * pose_std + pose_mean when given.  Frames of a single window are copied
    bit for bit (or equal normalization.denormalize bit for bit)."""
    from ._native import check, lib
    F._check_dev(windows, pose_mean, pose_std, out)
    if windows.dim() != 3:
        raise ValueError(f'windows must be [n, T, Fd], got {tuple(windows.shape)}')
    n, T, Fd = windows.shape
    if not 0 <= overlap <= T // 2:
        raise ValueError(f'overlap {overlap} outside [0, T/2 = {T // 2}]')
    if (pose_mean is None) != (pose_std is None):
        raise ValueError('pose_mean and pose_std come together')
    windows = windows.contiguous()
    frames = (n - 1) * (T - overlap) + T if n else 0
    if out is None:
        out = torch.empty(frames, Fd, device=windows.device)
    elif tuple(out.shape) != (frames, Fd) or not out.is_contiguous():
        raise ValueError(f'out must be a contiguous [{frames}, {Fd}] tensor')
    if pose_mean is not None:
        pose_mean, pose_std = pose_mean.to(windows.device).contiguous(), pose_std.to(windows.device).contiguous()
        if pose_mean.numel() != Fd or pose_std.numel() != Fd:
            raise ValueError(f'pose_mean and pose_std must have {Fd} entries')
    check(lib.a2m_track_blend_f32(F._p(windows), n, T, Fd, int(overlap), F._p(pose_mean), F._p(pose_std),
                                  F._p(out), F._stream()), value_error=True)
    return out


def track_starts(n_feature_frames, overlap=16, time=4.3, fs_new=15):
    """Feature-frame starts k * (T - overlap) * interval of every window that fits into a
    recording of n_feature_frames audio/log_mel_512 frames -> (starts int64, window, interval, T)."""
    import numpy as np
    from .windowing import window_index
    _, window, interval = window_index(n_feature_frames, 'audio/log_mel_512', fs_new, time)
    T = (window + interval - 1) // interval
    if not 0 <= overlap <= T // 2:
        raise ValueError(f'overlap {overlap} outside [0, T/2 = {T // 2}]')
    if n_feature_frames < window:
        raise ValueError(f'the recording has {n_feature_frames} feature frames; one window needs {window}')
    step = (T - overlap) * interval
    n = (n_feature_frames - window) // step + 1
    return step * np.arange(n, dtype=np.int64), window, interval, T


@torch.no_grad()
def generate_track(generator, wave, sr, overlap=16, batch=64, time=4.3, fs_new=15, audio_mean=None,
                   audio_std=None, pose_mean=None, pose_std=None, resample_to=None,
                   res_type='kaiser_best', **mel_kwargs):
    """A recording of any length to one continuous track: wave [S] (device) -> poses [F, 104].
    generate_from_wave returns separate windows, which jump at every border when laid end to end;
    here the windows start (T - overlap) pose frames apart (feature frame k * (T - overlap) *
    interval, as many as fit; ValueError when not even one does), the generator runs on at most
    `batch` of them per call, and a2m_track_blend_f32 cross-fades each overlap and applies
    pose_mean / pose_std in one pass: F = (n - 1)(T - overlap) + T.  The other arguments are
    generate_from_wave's.  overlap = 0 is the concatenation of generate_from_wave's windows."""
    from .pats_audio import log_mel_512_windows, num_frames, resample
    if batch < 1:
        raise ValueError('batch must be >= 1')
    if resample_to is not None:
        wave, sr = resample(wave, sr, resample_to, res_type), resample_to
    starts, window, interval, _ = track_starts(num_frames(wave.shape[-1], 2048, 512, True), overlap,
                                               time, fs_new)
    poses = []
    for i in range(0, len(starts), batch):
        audio = log_mel_512_windows(wave, sr, starts[i:i + batch], window, interval, audio_mean,
                                    audio_std, **mel_kwargs)
        poses.append(generate(generator, audio))
    windows = poses[0] if len(poses) == 1 else torch.cat(poses)
    return blend_track(windows, overlap, pose_mean, pose_std)


def generate_video(generator, wave, sr, output_fn, overlap=16, pose_mean=None, pose_std=None, quality=90,
                   track_kwargs=None, **video_kwargs):
    """A recording to a video with sound in one call: generate_track(generator, wave, sr, overlap,
    pose_mean=, pose_std=, **track_kwargs) -> planar_frames -> a2m.video.save_pose_avi(track,
    output_fn, wave, sr, quality, **video_kwargs), the same `wave` as the sound track (cut to the
    picture's duration).  output_fn must end in .avi.  Returns the number of frames."""
    from . import video
    video._avi_name(output_fn)
    track = generate_track(generator, wave, sr, overlap=overlap, pose_mean=pose_mean, pose_std=pose_std,
                           **(track_kwargs or {}))
    return video.save_pose_avi(planar_frames(track[None])[0], output_fn, wave=wave, sr=sr, quality=quality,
                               **video_kwargs)


class TrackBlendStream:
    """blend_track for windows that arrive a few at a time (a2m_track_blend_stream_f32): the
    concatenation of every push() and of close() equals blend_track(all windows) bit for bit.

    push(windows [m, T, Fd]) -> [m (T - overlap), Fd], the frames those windows make final (each
    window's head cross-faded with the carried tail of the one before); close() -> [overlap, Fd],
    the last window's tail, unblended.  The tail [overlap, Fd] is device state allocated here."""

    def __init__(self, T, Fd, overlap, pose_mean=None, pose_std=None, device='cuda'):
        if not 0 <= overlap <= T // 2:
            raise ValueError(f'overlap {overlap} outside [0, T/2 = {T // 2}]')
        if (pose_mean is None) != (pose_std is None):
            raise ValueError('pose_mean and pose_std come together')
        self.T, self.Fd, self.overlap, self.device = int(T), int(Fd), int(overlap), torch.device(device)
        self.mean = None if pose_mean is None else pose_mean.to(self.device, torch.float32).contiguous()
        self.std = None if pose_std is None else pose_std.to(self.device, torch.float32).contiguous()
        if self.mean is not None and (self.mean.numel() != self.Fd or self.std.numel() != self.Fd):
            raise ValueError(f'pose_mean and pose_std must have {self.Fd} entries')
        self.tail = torch.zeros(max(self.overlap, 1), self.Fd, device=self.device)
        self.windows, self.closed = 0, False

    def frames(self, m, flush=False):
        return m * (self.T - self.overlap) + (self.overlap if flush else 0)

    def _call(self, windows, m, flush, out):
        from ._native import check, lib
        n = self.frames(m, flush)
        if out is None:
            out = torch.empty(n, self.Fd, device=self.device)
        elif tuple(out.shape) != (n, self.Fd) or not out.is_contiguous() or out.dtype != torch.float32:
            raise ValueError(f'out must be a contiguous float32 [{n}, {self.Fd}] tensor')
        F._check_dev(self.tail, windows, out)
        check(lib.a2m_track_blend_stream_f32(F._p(windows), m, self.T, self.Fd, self.overlap, F._p(self.tail),
                                             int(self.windows > 0), int(flush), F._p(self.mean), F._p(self.std),
                                             F._p(out), F._stream()), value_error=True)
        self.windows += m
        return out

    def push(self, windows, out=None):
        if self.closed:
            raise ValueError('the stream is closed')
        if windows.dim() != 3 or tuple(windows.shape[1:]) != (self.T, self.Fd) or windows.dtype != torch.float32:
            raise ValueError(f'windows must be float32 [m, {self.T}, {self.Fd}], got {tuple(windows.shape)}')
        return self._call(windows.contiguous(), windows.shape[0], False, out)

    def close(self, out=None):
        if self.closed:
            raise ValueError('the stream is closed')
        if not self.windows:
            raise ValueError('no window was pushed: there is no tail to flush')
        self.closed = True
        return self._call(None, 0, True, out)


class TrackStream:
    """generate_track for audio that arrives as it is produced: the concatenation of every push()
    and of close() equals generate_track(generator, whole recording, sr, ...) (bit for bit where
    the generator is), whatever the chunking.

    push(samples [s]) -> [f, Fd] (device; f may be 0), the pose frames that became final: samples
    go through the optional pats_audio.ResampleStream and the pats_audio.MelWindowStream; the
    generator runs on at most `batch` due windows per call, in order; a2m_track_blend_stream_f32
    cross-fades each window's head with the carried tail of the one before and de-normalises.
    close() -> [f, Fd]: the windows that fit only the final length, then the last window's
    `overlap` tail frames; ValueError, as generate_track, when not one window fitted.

    The generator is not causal within a window, so a pose frame is final only once its window's
    audio is complete: frames come T - overlap at a time, up to one window (`time` seconds) behind
    the audio.  Samples may be a device tensor, a host tensor or numpy.  Read-only counters:
    samples_in, windows_out, frames_out."""

    def __init__(self, generator, sr, overlap=16, batch=1, time=4.3, fs_new=15, audio_mean=None,
                 audio_std=None, pose_mean=None, pose_std=None, resample_to=None, res_type='kaiser_best',
                 max_chunk=16384, device='cuda', pose_feats=None, **mel_kwargs):
        from .pats_audio import MelWindowStream, ResampleStream
        if batch < 1:
            raise ValueError('batch must be >= 1')
        if (pose_mean is None) != (pose_std is None):
            raise ValueError('pose_mean and pose_std come together')
        self.generator, self.batch = generator, int(batch)
        self.rs = None
        if resample_to is not None:
            self.rs = ResampleStream(sr, resample_to, res_type, max_chunk=max_chunk, device=device)
            sr = resample_to
        self.mel = MelWindowStream(sr, overlap, time, fs_new, audio_mean, audio_std, max_chunk=max_chunk,
                                   device=device, **mel_kwargs)
        self.device, self.T, self.overlap = self.mel.device, self.mel.T, self.mel.overlap
        if pose_feats is None and pose_mean is not None:
            pose_feats = pose_mean.numel()
        if pose_feats is None:
            pose_feats = generator.body_feats + generator.hand_feats    # SelfAttention_G's [B, T, 104]
        self.blend = TrackBlendStream(self.T, pose_feats, self.overlap, pose_mean, pose_std, self.device)
        self.Fd = self.blend.Fd
        self._samples_in, self._frames_out, self.closed = 0, 0, False

    samples_in = property(lambda self: self._samples_in)
    windows_out = property(lambda self: self.mel.windows_out)
    frames_out = property(lambda self: self._frames_out)

    def _blend(self, audio, flush):
        """Windows audio [m, T, n_mels] -> the frames they make final [m (T - overlap) (+ overlap), Fd]."""
        m = audio.shape[0]
        out = torch.empty(self.blend.frames(m, flush), self.Fd, device=self.device)
        at = 0
        for i in range(0, m, self.batch):
            pose = self.generator(audio[i:i + self.batch])[0]
            n = self.blend.frames(pose.shape[0], False)
            self.blend.push(pose, out=out[at:at + n])
            at += n
        if flush:
            self.blend.close(out=out[at:])
        self._frames_out += out.shape[0]
        return out

    @torch.no_grad()
    def push(self, samples):
        if self.closed:
            raise ValueError('the stream is closed')
        self._samples_in += len(samples)
        with torch.cuda.device(self.device):
            if self.rs is not None:
                samples = self.rs.push(samples)
            return self._blend(self.mel.push(samples), False)

    @torch.no_grad()
    def close(self):
        if self.closed:
            raise ValueError('the stream is closed')
        self.closed = True
        with torch.cuda.device(self.device):
            parts = []
            if self.rs is not None:
                parts.append(self._blend(self.mel.push(self.rs.close()), False))
            last = self.mel.close()
            if self.mel.windows_out == 0:
                from .pats_audio import num_frames
                nf = num_frames(self.mel.samples_in, 2048, 512, True) if self.mel.samples_in else 0
                raise ValueError(f'the recording has {nf} feature frames; one window needs {self.mel.window}')
            parts.append(self._blend(last, True))
            parts = [p for p in parts if p.shape[0]]
            return parts[0] if len(parts) == 1 else \
                torch.cat(parts) if parts else torch.empty(0, self.Fd, device=self.device)


class VideoStream:
    """generate_video for audio that arrives as it is produced: takes generate_video's arguments
    without the wave; push(samples) feeds a TrackStream, appends the chunk's PCM to the AVI's sound
    track (so the sound always runs ahead of the frames it accompanies), and renders, encodes and
    writes every frame that became final; close() writes the tail and returns the frame count.
    The file equals generate_video's for the same recording byte for byte."""

    def __init__(self, generator, sr, output_fn, overlap=16, pose_mean=None, pose_std=None, quality=90,
                 track_kwargs=None, fps=None, chunk=64, polylines=None, colors=None, img_size=(3000, 1000),
                 scale=0.5, line_width=None, background=(255, 255, 255)):
        import numpy as np
        from . import avi, jpeg, video
        video._avi_name(output_fn)
        if chunk < 1:
            raise ValueError('chunk must be >= 1')
        self.track = TrackStream(generator, sr, overlap=overlap, pose_mean=pose_mean, pose_std=pose_std,
                                 **(track_kwargs or {}))
        self.polylines = video.REFERENCE_POLYLINES if polylines is None else polylines
        self.canvas, self.scale, self.line_width, self.chunk = img_size, scale, line_width, int(chunk)
        self.ycc = video.rgb_to_ycbcr_full(np.asarray(video._colors(self.polylines, colors), np.uint8).reshape(-1, 3))
        self.bg = video.rgb_to_ycbcr_full(np.asarray(background, np.uint8))
        W, H = int(round(img_size[0] * scale)), int(round(img_size[1] * scale))
        self.qt = jpeg.quant_tables(quality)
        self.writer = avi.AVIWriter(output_fn, W, H, video.FPS if fps is None else fps, audio_rate=sr)
        self.header = jpeg.jpeg_header(W, H, self.qt)
        self._dev, self._shape = None, (3, H, W)

    frames = property(lambda self: self.writer.frames)

    def _write(self, track):
        from . import jpeg, video
        if not track.shape[0]:
            return
        kp = planar_frames(track[None])[0][:, None]          # [f, 1, 2, K], as save_pose_avi draws it
        for i in range(0, kp.shape[0], self.chunk):
            part = kp[i:i + self.chunk]
            if self._dev is None or self._dev.shape[0] != part.shape[0]:
                self._dev = torch.empty(part.shape[0], *self._shape, dtype=torch.uint8, device=part.device)
            video.render_poses(part, self.polylines, self.ycc, self.canvas, self.scale, self.line_width, None,
                               self.bg, out=self._dev)
            buf, off = jpeg.encode_scans(self._dev, self.qt)
            for n in range(part.shape[0]):
                self.writer.write_frame(self.header, buf[off[n]:off[n + 1]].data, jpeg.EOI)

    def push(self, samples):
        from . import avi
        self.writer.add_audio(avi.pcm16(samples))
        self._write(self.track.push(samples))

    def close(self):
        try:
            self._write(self.track.close())
        finally:
            self.writer.close()
        return self.writer.frames


def planar_frames(pose):
    B, T, _ = pose.shape
    return pose.reshape(B, T, 2, -1)


class GraphedGenerator:
    """Fixed-shape eval forward of SelfAttention_G as four HIP graphs replayed on two streams:

        trunk  (main):  prologue() -> audio encoder -> UNet -> feats
        body   (side):  body decoder branch -> out[..., :20]      } concurrent after the fork
        hand   (main):  hand decoder branch -> out[..., 20:]      }
        losses (main):  after the join, pose losses of out

    One graph with both branches inside leaves the second branch waiting: on ROCm 7 its
    first kernel started 350-500 us after the fork in every replay we traced (r02 step
    trace).  Separate single-stream graphs start both branches at the fork (traced), but at
    B = 64 the branches' kernels already fill the chip, so the bench step measured no faster
    (3.19 vs 3.14 ms; bench.py --branch-graphs): kept as the serving-loop API, not the bench
    default.

    `prologue` produces the [B, T, 128] generator input from static device buffers (e.g. the
    bench's HIP log-mel over resident waveforms); call() replays and returns the static
    [B, T, 104] output and the losses list (valid until the next call)."""

    def __init__(self, generator, prologue):
        g = generator
        assert not g.training, 'GraphedGenerator replays the eval forward'
        self.g, self.prologue = g, prologue
        dev = next(g.parameters()).device
        self.main = torch.cuda.Stream(dev)
        self.side = torch.cuda.Stream(dev)
        self.fork, self.join = torch.cuda.Event(), torch.cuda.Event()
        self.static = {}
        with torch.no_grad():
            # warm-up: every workspace / cache is created on the stream that will replay it
            for _ in range(2):
                self._trunk()
                self._branches(eager=True)
                self._losses()
            torch.cuda.synchronize(dev)
            # the main-stream graphs share one pool (they replay in capture order on one
            # stream); the body graph runs concurrently with the hand graph, so its
            # temporaries must not alias theirs: a pool of its own
            pool, side_pool = torch.cuda.graph_pool_handle(), torch.cuda.graph_pool_handle()
            self.graphs = {}
            for name, stream, fn, pl in (('trunk', self.main, self._trunk, pool),
                                         ('body', self.side, lambda: self._branch('body'), side_pool),
                                         ('hand', self.main, lambda: self._branch('hand'), pool),
                                         ('losses', self.main, self._losses, pool)):
                gr = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gr, pool=pl, stream=stream):
                    fn()
                self.graphs[name] = gr
        torch.cuda.synchronize(dev)

    def _trunk(self):
        with torch.cuda.stream(self.main):
            x = self.prologue()
            B, T, _ = x.shape
            self.static['feats'] = self.g.unet(self.g.audio_encoder(x))
            if 'out' not in self.static:
                self.static['out'] = torch.empty(B, T, self.g.body_feats + self.g.hand_feats,
                                                 device=x.device)

    def _branch(self, part):
        stream = self.side if part == 'body' else self.main
        with torch.cuda.stream(stream):
            f0 = 0 if part == 'body' else self.g.body_feats
            self.g._branch(part, self.static['feats'], self.static['out'], f0)

    def _branches(self, eager):
        self.fork.record(self.main)
        self.side.wait_event(self.fork)
        self._branch('body')
        self._branch('hand')
        self.join.record(self.side)
        self.main.wait_event(self.join)

    def _losses(self):
        with torch.cuda.stream(self.main):
            self.static['losses'] = F.pose_losses(self.static['out'], None)

    def __call__(self):
        cur = torch.cuda.current_stream()
        self.main.wait_stream(cur)
        with torch.cuda.stream(self.main):
            self.graphs['trunk'].replay()
            self.fork.record(self.main)
        self.side.wait_event(self.fork)
        with torch.cuda.stream(self.side):
            self.graphs['body'].replay()
            self.join.record(self.side)
        with torch.cuda.stream(self.main):
            self.graphs['hand'].replay()
            self.main.wait_event(self.join)
            self.graphs['losses'].replay()
        cur.wait_stream(self.main)
        return self.static['out'], [self.static['losses'][1]]
