"""RIFF AVI 1.0 with Motion-JPEG video and 16-bit PCM sound, written and read back with `struct`
alone (generate_motion_video.py:203-207 hands this to ffmpeg).

  AVIWriter(path, W, H, fps, audio_rate)   hdrl (avih, a 'vids'/MJPG stream, an optional
                                           'auds' PCM mono s16le stream), movi ('00dc' per frame,
                                           each followed by that frame's '01wb'), idx1;
                                           the sound whole (set_audio) or as it comes (add_audio)
  pcm16(wave)                             float [-1, 1] -> int16 samples
  read_avi(path)                           the files AVIWriter writes -> frames, sound, rates
  save_video_from_audio_video(wav, avi, out)   the reference's function: a PCM .wav under the
                                           picture of one of our .avi files

Chunks are padded to even length; the RIFF, LIST and header sizes are patched at close().  A file
stays below 2 GiB (AVI 1.0; OpenDML is out of scope): the writer raises ValueError before a frame
would take it past that.
"""
import struct
import wave as _wave

import numpy as np

FPS = (30000, 2002)          # the reference's ffmpeg input rate (a2m.video.FPS)
LIMIT = 2 ** 31 - 1          # the largest file an AVI 1.0 reader must accept
AVIF_HASINDEX, AVIF_ISINTERLEAVED, AVIIF_KEYFRAME = 0x10, 0x100, 0x10


def pcm16(wave):
    """float samples in [-1, 1] (numpy, sequence or tensor; mono) -> little-endian int16: clipped,
    scaled by 32767, rounded to nearest."""
    if hasattr(wave, 'detach'):
        wave = wave.detach().cpu().numpy()
    w = np.asarray(wave, np.float64)
    if w.ndim != 1:
        raise ValueError(f'the sound track is mono: wave must be [S], got {w.shape}')
    return np.rint(np.clip(w, -1.0, 1.0) * 32767.0).astype('<i2')


def _chunk(fourcc, payload):
    return fourcc + struct.pack('<I', len(payload)) + payload + (b'\x00' if len(payload) & 1 else b'')


def _list(kind, payload):
    return b'LIST' + struct.pack('<I', len(payload) + 4) + kind + payload


class AVIWriter:
    """write_frame(*pieces) appends one JPEG file (its pieces are written one after the other) as
    a '00dc' chunk and, with audio_rate, the frame's share of the samples given to set_audio (the
    whole track, before the first frame) or add_audio (in pieces, ahead of the frames) as a
    '01wb' chunk: frame i holds samples [floor(i sr scale / rate), floor((i + 1) sr scale / rate)),
    so no sample is lost or doubled, and the sound ends with the picture."""

    def __init__(self, path, W, H, fps=FPS, audio_rate=None):
        if not str(path).endswith('.avi'):
            raise ValueError(f'the video is written as AVI: the path must end in .avi, got {path!r}')
        if not (1 <= W <= 65535 and 1 <= H <= 65535):
            raise ValueError(f'a Motion-JPEG frame is 1..65535 pixels a side, got {W} x {H}')
        rate, scale = int(fps[0]), int(fps[1])
        if rate < 1 or scale < 1:
            raise ValueError(f'fps is (rate, scale), both positive, got {fps!r}')
        if audio_rate is not None and not 1 <= int(audio_rate) <= 2 ** 31 - 1:
            raise ValueError(f'audio_rate must be a positive sample rate, got {audio_rate!r}')
        self.W, self.H, self.rate, self.scale = int(W), int(H), rate, scale
        self.audio_rate = None if audio_rate is None else int(audio_rate)
        self.frames, self.samples = 0, 0
        self._audio = np.zeros(0, '<i2')
        self._audio_off, self._streamed = 0, False   # add_audio: samples dropped so far; sound arrives in pieces
        self._index = []                   # (fourcc, offset from the 'movi' fourcc, size)
        self._largest = [0, 0]               # largest video / audio chunk
        self._closed = False
        self.f = open(path, 'wb')
        self.f.write(self._header())
        self._movi = self._size = self.f.tell()      # _movi: just past the 'movi' fourcc

    def set_audio(self, samples):
        """int16 samples (pcm16 output) of the whole track, before the first frame."""
        if self.audio_rate is None:
            raise ValueError('the writer was opened without audio_rate')
        if self.frames:
            raise ValueError('set_audio comes before the first frame')
        self._audio = np.ascontiguousarray(samples, '<i2').reshape(-1)
        self._audio_off, self._streamed = 0, False

    def add_audio(self, samples):
        """Appends int16 samples (pcm16 output) to the track, at any time before close(): the
        streaming form of set_audio.  The sound must run ahead of the picture: write_frame raises
        when a frame's share of the samples has not all arrived.  Samples already written out are
        dropped, so a long stream holds only what is ahead of the picture."""
        if self.audio_rate is None:
            raise ValueError('the writer was opened without audio_rate')
        if self._closed:
            raise ValueError('the file is closed')
        new = np.ascontiguousarray(samples, '<i2').reshape(-1)
        used = max(0, min(self._share(self.frames) - self._audio_off, len(self._audio))) if self._streamed else 0
        self._audio = np.concatenate([self._audio[used:], new])
        self._audio_off += used
        self._streamed = True

    def _share(self, i):
        return i * self.audio_rate * self.scale // self.rate

    def _header(self):
        n_streams = 1 if self.audio_rate is None else 2
        per_sec = -(-self._largest[0] * self.rate // self.scale) + 2 * (self.audio_rate or 0)
        avih = struct.pack('<14I', (1000000 * self.scale + self.rate // 2) // self.rate,
                           min(per_sec, 2 ** 32 - 1),
                           0, AVIF_HASINDEX | (AVIF_ISINTERLEAVED if n_streams == 2 else 0), self.frames, 0,
                           n_streams, self._largest[0], self.W, self.H, 0, 0, 0, 0)
        strh = struct.pack('<4s4sIHHIIIIIIII4H', b'vids', b'MJPG', 0, 0, 0, 0, self.scale, self.rate, 0,
                           self.frames, self._largest[0], 0xFFFFFFFF, 0, 0, 0, self.W, self.H)
        strf = struct.pack('<IiiHH4sIiiII', 40, self.W, self.H, 1, 24, b'MJPG', min(self.W * self.H * 3, 2 ** 32 - 1),
                           0, 0, 0, 0)
        body = _chunk(b'avih', avih) + _list(b'strl', _chunk(b'strh', strh) + _chunk(b'strf', strf))
        if n_streams == 2:
            strh = struct.pack('<4s4sIHHIIIIIIII4H', b'auds', b'\0\0\0\0', 0, 0, 0, 0, 1, self.audio_rate,
                               0, self.samples, self._largest[1], 0xFFFFFFFF, 2, 0, 0, 0, 0)
            strf = struct.pack('<HHIIHH', 1, 1, self.audio_rate, 2 * self.audio_rate, 2, 16)
            body += _list(b'strl', _chunk(b'strh', strh) + _chunk(b'strf', strf))
        hdrl = _list(b'hdrl', body)
        movi = getattr(self, '_size', 0) - getattr(self, '_movi', 0)
        riff = 4 + len(hdrl) + 12 + movi + ((8 + 16 * len(self._index)) if self._closed else 0)
        return b'RIFF' + struct.pack('<I', riff) + b'AVI ' + hdrl + b'LIST' + struct.pack('<I', movi + 4) + b'movi'

    def _append(self, fourcc, pieces, which):
        size = sum(len(p) for p in pieces)
        self._index.append((fourcc, self._size - self._movi + 4, size))
        self.f.write(fourcc + struct.pack('<I', size))
        for p in pieces:
            self.f.write(p)
        if size & 1:
            self.f.write(b'\x00')
        self._size += 8 + size + (size & 1)
        self._largest[which] = max(self._largest[which], size)

    def write_frame(self, *pieces):
        if self._closed:
            raise ValueError('the file is closed')
        size = sum(len(p) for p in pieces)
        chunks, sound = 8 + size + (size & 1), b''
        if self.audio_rate is not None:
            lo, hi = self._share(self.frames) - self._audio_off, self._share(self.frames + 1) - self._audio_off
            if self._streamed and hi > len(self._audio):
                raise ValueError(f'frame {self.frames} takes samples up to {hi + self._audio_off}, but only '
                                 f'{len(self._audio) + self._audio_off} have been added: add_audio runs ahead '
                                 f'of the frames')
            sound = self._audio[lo:hi].tobytes()
            chunks += 8 + len(sound)
        entries = len(self._index) + (1 if self.audio_rate is None else 2)
        if self._size + chunks + 8 + 16 * entries > LIMIT:
            raise ValueError(f'frame {self.frames} would take the file past 2 GiB, the limit of AVI 1.0; '
                             f'write a shorter track, a smaller canvas or a lower quality')
        self._append(b'00dc', pieces, 0)
        if self.audio_rate is not None:
            self._append(b'01wb', (sound,), 1)
            self.samples += len(sound) // 2
        self.frames += 1

    def close(self):
        if self._closed:
            return
        self._closed = True
        idx = b''.join(struct.pack('<4sIII', cc, AVIIF_KEYFRAME, off, size) for cc, off, size in self._index)
        self.f.write(_chunk(b'idx1', idx))
        self.f.seek(0)
        self.f.write(self._header())
        self.f.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


def _unsupported(path, what):
    return ValueError(f'{path!r}: {what}; supported are RIFF AVI 1.0 files as a2m.avi.AVIWriter writes them '
                      f'(one MJPG video stream, at most one PCM mono 16-bit audio stream, an idx1 index)')


def read_avi(path):
    """-> dict(W, H, fps (rate, scale), frames [bytes], audio_rate or None, audio int16 [S],
    index [(fourcc, offset, size)], movi: file position of the 'movi' fourcc)."""
    with open(path, 'rb') as f:
        data = f.read()
    if len(data) < 12 or data[:4] != b'RIFF' or data[8:12] != b'AVI ':
        raise _unsupported(path, 'not a RIFF AVI file')
    if struct.unpack('<I', data[4:8])[0] + 8 != len(data):
        raise _unsupported(path, 'the RIFF size does not match the file')
    out = dict(frames=[], audio_rate=None, index=[], movi=None)
    sound, streams = [], []

    def walk(lo, hi, depth):
        while lo + 8 <= hi:
            cc, size = data[lo:lo + 4], struct.unpack('<I', data[lo + 4:lo + 8])[0]
            body = lo + 8
            if body + size > hi:
                raise _unsupported(path, f'chunk {cc!r} at {lo} runs past its parent')
            if cc == b'LIST':
                kind = data[body:body + 4]
                if kind == b'movi':
                    out['movi'] = body
                walk(body + 4, body + size, depth + 1)
            elif cc == b'strh':
                streams.append(struct.unpack('<4s4sIHHIIIIIIII4H', data[body:body + 56]))
            elif cc == b'strf' and not streams:
                raise _unsupported(path, 'a stream format without a stream header')
            elif cc == b'strf' and streams[-1][0] == b'vids':
                _, out['W'], out['H'], _, _, comp = struct.unpack('<IiiHH4s', data[body:body + 20])
                if comp != b'MJPG':
                    raise _unsupported(path, f'video compression {comp!r}')
                out['fps'] = (streams[-1][7], streams[-1][6])
            elif cc == b'strf' and streams[-1][0] == b'auds':
                tag, channels, rate, _, _, bits = struct.unpack('<HHIIHH', data[body:body + 16])
                if (tag, channels, bits) != (1, 1, 16):
                    raise _unsupported(path, f'audio format tag {tag}, {channels} channel(s), {bits} bits')
                out['audio_rate'] = rate
            elif cc == b'00dc':
                out['frames'].append(data[body:body + size])
            elif cc == b'01wb':
                sound.append(data[body:body + size])
            elif cc == b'idx1':
                entries = [struct.unpack('<4sIII', data[body + 16 * k:body + 16 * k + 16])
                           for k in range(size // 16)]
                out['index'] = [(cc4, off, n) for cc4, _, off, n in entries]
            lo = body + size + (size & 1)

    walk(12, len(data), 0)
    if 'fps' not in out or out['movi'] is None or len(streams) > 2:
        raise _unsupported(path, 'no MJPG video stream, no movi list or more than two streams')
    out['audio'] = np.frombuffer(b''.join(sound), '<i2')
    return out


def read_wav(path):
    """A PCM .wav -> (int16 mono samples, rate); several channels are averaged."""
    try:
        with _wave.open(str(path), 'rb') as w:
            channels, width, rate, n = w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()
            raw = w.readframes(n)
    except (_wave.Error, EOFError) as e:
        raise ValueError(f'{path!r}: {e}; supported are uncompressed PCM .wav files of 16-bit samples')
    if width != 2:
        raise ValueError(f'{path!r} has {8 * width}-bit samples; supported are uncompressed PCM .wav files '
                         f'of 16-bit samples')
    pcm = np.frombuffer(raw, '<i2').reshape(-1, channels)
    if channels > 1:
        pcm = np.rint(pcm.astype(np.float64).mean(1)).astype('<i2')
    return pcm.reshape(-1), rate


def save_video_from_audio_video(audio_input_path, input_video_path, output_video_path):
    """generate_motion_video.save_video_from_audio_video without ffmpeg: the sound of a PCM .wav
    (16-bit; channels averaged to mono) under the picture of an .avi that AVIWriter wrote, into
    a new .avi.  The sound is cut to the picture's duration; an audio stream the input video
    already has is dropped.  Returns the number of frames."""
    for path, ext in ((audio_input_path, '.wav'), (input_video_path, '.avi'), (output_video_path, '.avi')):
        if not str(path).endswith(ext):
            raise ValueError(f'{path!r}: supported are a PCM .wav as the sound, and .avi files as a2m writes '
                             f'them as the picture and the output')
    pcm, rate = read_wav(audio_input_path)
    video = read_avi(input_video_path)
    with AVIWriter(output_video_path, video['W'], video['H'], video['fps'], audio_rate=rate) as w:
        w.set_audio(pcm)
        for frame in video['frames']:
            w.write_frame(frame)
        return w.frames
