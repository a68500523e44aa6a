/*
 * a2m.h -- C-ABI of liba2m_hip.so, the MI355X (gfx950) audio -> 2-D pose hot path.
 *
 * Every entry point takes caller-owned DEVICE pointers, explicit sizes / element strides
 * and a hipStream_t passed as void*.  Nothing allocates device memory: scratch comes from
 * the caller through (ws, ws_bytes).  Calls are stream-ordered and reentrant (no hidden
 * global state besides the thread-local error string), so they are safe to capture into
 * a hipGraph.  Return value: 0 = ok, A2M_EINVAL (bad shape / argument), A2M_EHIP (HIP
 * error), A2M_EWS (workspace too small); a2m_last_error() holds the message.
 *
 * The reference (Xukai-UoA/Audio-to-Motion-Generation) is pure Python/PyTorch; each entry
 * cites the reference code it replaces (file:line, paths relative to the reference root).
 * Tensor layouts follow the reference's PyTorch layouts: [B][C][T] for 1-D feature maps,
 * [B][C][H][W] for 2-D, [B][T][F] for pose / mel.
 */
#ifndef A2M_H_
#define A2M_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define A2M_OK 0
#define A2M_EINVAL -1
#define A2M_EHIP -2
#define A2M_EWS -3

/* activation codes used by the *_fwd entry points */
#define A2M_ACT_NONE 0
#define A2M_ACT_RELU 1
#define A2M_ACT_LRELU 2

const char* a2m_last_error(void);
int a2m_version(void);

/* ---------------------------------------------------------------- log-mel front end
 * Replaces pose_video/mel_features.py:192-223 (log_mel_spectrogram) with its helpers
 * frame :21, periodic_hann :48, stft_magnitude :71, spectrogram_to_mel_matrix :114.
 * Plan = periodic Hann window + FFT twiddles + banded (CSR) mel filterbank, built on the
 * HOST in float64 exactly as the reference builds its matrix, then copied by the caller
 * to device memory once.  a2m_logmel_plan_build returns A2M_EINVAL with the reference's
 * ValueError text for bad band edges (mel_features.py:156-163).
 */
int64_t a2m_logmel_num_frames(int64_t n_samples, int32_t window, int32_t hop);
int a2m_logmel_geometry(int32_t sample_rate, double window_secs, double hop_secs,
                        int32_t* window, int32_t* hop, int32_t* fft_len);
size_t a2m_logmel_plan_bytes(int32_t sample_rate, double window_secs, double hop_secs,
                             int32_t n_mels, double lower_hz, double upper_hz);
int a2m_logmel_plan_build(int32_t sample_rate, double window_secs, double hop_secs,
                          int32_t n_mels, double lower_hz, double upper_hz,
                          void* host_plan, size_t plan_bytes);
/* wave[c][s] at wave + c*clip_stride + s (float32, n_samples per clip);
 * out[c][f][m] at out + (c*n_frames + f)*n_mels + m, n_frames = a2m_logmel_num_frames() */
int a2m_logmel_f32(const float* wave, int64_t n_clips, int64_t clip_stride, int64_t n_samples,
                   int32_t window, int32_t hop, int32_t fft_len, int32_t n_mels,
                   const void* dev_plan, float log_offset, float* out, void* stream);

/* ---------------------------------------------------------------- PATS audio features
 * audio/log_mel_512 and audio/log_mel_400 from a waveform (pats/data_loading/audio.py:58-120),
 * i.e. librosa.feature.melspectrogram: frames of n_fft samples every `hop`, a periodic Hann of
 * win_length centred in the frame, |rfft|^power (1 or 2, DC kept), a Slaney mel filterbank
 * (htk=False; slaney_norm != 0 scales each triangle to unit area), exact zeros replaced by eps,
 * natural log.  The plan is built on the HOST in float64 and copied to the device by the caller,
 * like the a2m_logmel_* one; bad band edges (fmax above Nyquist, ...) give A2M_EINVAL.
 *   log_mel_512: n_fft 2048, hop 512, win_length 2048, 128 mels, 0..sr/2, norm, power 2, centred
 *   log_mel_400: sr 16000, n_fft 512, hop 160, win_length 400, 64 mels, 125..7500, no norm,
 *                power 1, not centred */
#define A2M_PAD_REFLECT 0  /* numpy.pad 'reflect': mirrored without repeating the edge sample */
#define A2M_PAD_CONSTANT 1 /* zeros */
size_t a2m_pats_audio_plan_bytes(int32_t sample_rate, int32_t n_fft, int32_t hop, int32_t win_length,
                                 int32_t n_mels, double fmin, double fmax, int32_t slaney_norm,
                                 int32_t power);
int a2m_pats_audio_plan_build(int32_t sample_rate, int32_t n_fft, int32_t hop, int32_t win_length,
                              int32_t n_mels, double fmin, double fmax, int32_t slaney_norm,
                              int32_t power, void* host_plan, size_t plan_bytes);
/* the plan's filterbank as a dense basis[n_mels][1 + n_fft/2] (what librosa.filters.mel returns) */
int a2m_pats_audio_plan_filterbank(const void* host_plan, size_t plan_bytes, float* basis);
/* center != 0: n_fft/2 samples of padding on both sides, 1 + n_samples / hop frames;
 * otherwise 1 + (n_samples - n_fft) / hop, and 0 below n_fft samples */
int64_t a2m_pats_audio_num_frames(int64_t n_samples, int32_t n_fft, int32_t hop, int32_t center);
/* wave as for a2m_logmel_f32.  frame_ids == NULL: out[c][f][m], n_out = n_clips * n_frames.
 * Otherwise row r of out[n_out][n_mels] is source frame frame_ids[r] = clip * n_frames + frame
 * (device int64; an id out of range gives a row of NaN), so a window gather computes only the
 * frames it reads.  mean / std (both or neither, [n_mels]) standardise the output as
 * a2m_window_gather_f32 does.  Reflect padding needs n_samples > n_fft / 2.  No host
 * synchronisation: capturable into a HIP graph. */
int a2m_pats_audio_f32(const float* wave, int64_t n_clips, int64_t clip_stride, int64_t n_samples,
                       int32_t n_fft, int32_t hop, int32_t win_length, int32_t n_mels, int32_t power,
                       const void* dev_plan, int32_t center, int32_t pad_mode, float eps,
                       const int64_t* frame_ids, int64_t n_out, const float* mean, const float* std_,
                       float* out, void* stream);
/* The same features of a signal that arrives in pieces.  buf is a linear sliding device buffer
 * holding samples [base, base + len) of one unbounded signal (sample g at buf[g - base]);
 * n_total is the signal's length once its end is known, negative until then.  frame_ids (device
 * int64, required) are absolute frame indices of that signal: frame i spans samples
 * [i hop - n_fft/2, i hop + n_fft/2) when centred.  Padding about sample 0 is as offline
 * (reflection, or zeros under A2M_PAD_CONSTANT); about the end it applies only when n_total >= 0.
 * A frame that needs a sample the buffer does not hold and that is not a defined zero (before
 * `base`, not yet arrived, past an unknown end), or whose id lies outside the signal, gives a row
 * of NaN and reads nothing.  The per-frame arithmetic is the offline kernel's own code, so a frame
 * equals a2m_pats_audio_f32's of the whole signal bit for bit.  The frame loads are vector loads:
 * base must be a multiple of 4 samples and buf 16-byte aligned (compact the buffer by multiples of
 * the hop).  mean / std as above.  A2M_EINVAL: bad geometry, negative base / len / n_out, a
 * misaligned base or buf, mean without std, reflect padding with 0 <= n_total <= n_fft/2, a null
 * pointer with n_out > 0.  n_out = 0 returns A2M_OK.  No allocation, no host synchronisation:
 * capturable. */
int a2m_pats_audio_stream_f32(const float* buf, int64_t base, int64_t len, int64_t n_total, int32_t n_fft,
                              int32_t hop, int32_t win_length, int32_t n_mels, int32_t power,
                              const void* dev_plan, int32_t center, int32_t pad_mode, float eps,
                              const int64_t* frame_ids, int64_t n_out, const float* mean,
                              const float* std_, float* out, void* stream);

/* ---------------------------------------------------------------- waveform resampling
 * What librosa.core.resample did ahead of log_mel_400 (pats/data_loading/audio.py:88): band-limited
 * interpolation with a Kaiser-windowed sinc of num_zeros zero crossings, Kaiser parameter beta and
 * roll-off `rolloff` (resampy's kaiser_best: 64, 14.769656459379492, 0.9475937167399596;
 * kaiser_fast: 16, 8.555504641634386, 0.85).  With g = gcd(sr_in, sr_out), P = sr_in/g, Q = sr_out/g,
 * s = min(1, sr_out/sr_in), L = ceil(num_zeros / s), output t sits at input position t P / Q,
 * n_t = (t P) div Q, p_t = (t P) mod Q in 64-bit integers, and
 *   y[t] = sum_{k=-L+1..L} h_{p_t}[k] x[n_t + k],  x = 0 outside [0, n_samples),
 *   h_p[k] = s rolloff sinc(s rolloff tau) w(s tau / num_zeros),  tau = (p - k Q) / Q,
 *   w(u) = I0(beta sqrt(1 - u^2)) / I0(beta) for |u| < 1, else 0,
 * the continuous filter evaluated exactly (no interpolated table).  Output length
 * ceil(n_samples sr_out / sr_in).  The plan (the Q x 2L taps) is built on the HOST in float64, stored
 * as float32 and copied to the device by the caller, like the log-mel plans.  A2M_EINVAL: a rate or
 * num_zeros below 1, rolloff outside (0, 1], beta < 0, or a reduced ratio P/Q whose bank Q 2L
 * exceeds 2^21 floats (nearly coprime rates). */
int64_t a2m_resample_num_samples(int64_t n_samples, int32_t sr_in, int32_t sr_out);
size_t a2m_resample_plan_bytes(int32_t sr_in, int32_t sr_out, int32_t num_zeros, double beta,
                               double rolloff);
int a2m_resample_plan_build(int32_t sr_in, int32_t sr_out, int32_t num_zeros, double beta,
                            double rolloff, void* host_plan, size_t plan_bytes);
/* the reduced ratio, the half width and (bank != NULL) the dense bank[Q][2L]: row p holds h_p[k],
 * k = -L+1..L.  The layout inside the plan is the kernel's own. */
int a2m_resample_plan_bank(const void* host_plan, size_t plan_bytes, int32_t* P, int32_t* Q, int32_t* L,
                           float* bank);
/* wave as for a2m_logmel_f32; out[c][t] at out + c*out_stride + t, n_out =
 * a2m_resample_num_samples().  sr_in, sr_out and num_zeros are the plan's (the plan is device
 * memory, so the launch takes them again, as a2m_pats_audio_f32 takes its geometry).  Never reads
 * outside a clip's [0, n_samples).  A2M_EINVAL for null pointers, negative sizes, a wrong n_out, or
 * n_samples * Q beyond 62 bits.  No allocation, no host synchronisation: capturable. */
int a2m_resample_f32(const float* wave, int64_t n_clips, int64_t clip_stride, int64_t n_samples,
                     int32_t sr_in, int32_t sr_out, int32_t num_zeros, const void* dev_plan, float* out,
                     int64_t out_stride, int64_t n_out, void* stream);
/* Outputs t in [t_begin, t_begin + n_out) of the same formula for a signal that arrives in pieces:
 * out[t - t_begin] = y[t].  buf is a linear sliding device buffer holding samples [base, base + len)
 * (sample g at buf[g - base]); x[g] = 0 for g < 0, and for g >= n_total once the end is known
 * (n_total >= 0; negative: still open).  The tap loop is a2m_resample_f32's own code, so y[t]
 * equals the offline result bit for bit.  Never reads outside [base, base + len).  A2M_EINVAL: a
 * null pointer with n_out > 0, a negative base / len / t_begin / n_out, or an output whose taps
 * reach a sample that the buffer does not hold and that is not a defined zero.  n_out = 0 returns
 * A2M_OK.  No allocation, no host synchronisation: capturable. */
int a2m_resample_stream_f32(const float* buf, int64_t base, int64_t len, int64_t n_total, int32_t sr_in,
                            int32_t sr_out, int32_t num_zeros, const void* dev_plan, int64_t t_begin,
                            int64_t n_out, float* out, void* stream);

/* ---------------------------------------------------------------- convolutions
 * ConvNormRelu (model_layers.py:51-118) forward in eval mode: conv + bias, optional
 * BatchNorm (running stats; bn_w == NULL disables it), activation (A2M_ACT_*, LeakyReLU
 * slope), all fused into the MFMA implicit-GEMM epilogue.  Also used for nn.Linear
 * (kernel 1, T = rows) and 1x1 convs.  Element (b, c, t) of x lives at
 * x + b*xs_b + c*xs_c + t*xs_t, same for y; Tout = (Tin + 2*pad - ks)/stride + 1.
 */
int a2m_conv1d_fwd_f32(const float* x, int64_t xs_b, int64_t xs_c, int64_t xs_t,
                       int32_t B, int32_t Ci, int32_t Tin,
                       const float* w, const float* bias, int32_t Co, int32_t ks,
                       int32_t stride, int32_t pad,
                       const float* bn_w, const float* bn_b, const float* bn_rm,
                       const float* bn_rv, float bn_eps, int32_t act, float slope,
                       float* y, int64_t ys_b, int64_t ys_c, int64_t ys_t,
                       void* ws, size_t ws_bytes, void* stream);

/* ConvTranspose1D (model_layers.py:193-215): ConvTranspose1d(k, stride, pad, out_pad)
 * + BN + ReLU.  w is [Ci][Co][ks]; Tout = (Tin-1)*stride - 2*pad + ks + out_pad. */
int a2m_convt1d_fwd_f32(const float* x, int64_t xs_b, int64_t xs_c, int32_t B, int32_t Ci,
                        int32_t Tin, const float* w, const float* bias, int32_t Co, int32_t ks,
                        int32_t stride, int32_t pad, int32_t out_pad,
                        const float* bn_w, const float* bn_b, const float* bn_rm,
                        const float* bn_rv, float bn_eps, int32_t act, float slope,
                        float* y, int64_t ys_b, int64_t ys_c,
                        void* ws, size_t ws_bytes, void* stream);
/* Tap-chunked conv1d (stride 1, "same" padding 2*pad == ks-1): the forward of
 * model_layers.py ConvNormRelu(type='1d') / ResBlock convs (nn.Conv1d(k=3, s=1, p=1),
 * model_layers.py:75-120) without an im2col matrix.  Weights are packed once per weight version
 * by a2m_conv1d_tap_pack_f32 as [Co][Ci/chunk][ks][chunk] with chunk = a2m_conv1d_tap_chunk()
 * (the engine's k-tile at the current precision: 32 fp32 / bf16x6, 64 bf16); the GEMM's B
 * loader reads each chunk's x[b][c][t] window once and re-stores it shifted for every tap.
 * x: [B][Ci][T] with unit t stride and 16-byte aligned rows; T % 4 == 0 and 64 % T == 0 (the
 * tiles hold whole clips).  Epilogue (bias, BN-eval, activation) and output strides as
 * a2m_conv1d_fwd_f32. */
int32_t a2m_conv1d_tap_chunk(void);
int a2m_conv1d_tap_pack_f32(const float* w, int32_t Co, int32_t Ci, int32_t ks, int32_t chunk,
                            float* packed, void* stream);
int a2m_conv1d_tap_fwd_f32(const float* x, int64_t xs_b, int64_t xs_c, int32_t B, int32_t Ci,
                           int32_t T, const float* packed, int32_t chunk, const float* bias,
                           int32_t Co, int32_t ks, int32_t pad, const float* bn_w,
                           const float* bn_b, const float* bn_rm, const float* bn_rv, float bn_eps,
                           int32_t act, float slope, float* y, int64_t ys_b, int64_t ys_c,
                           int64_t ys_t, void* ws, size_t ws_bytes, void* stream);
/* G independent tap-chunked conv1d problems in one launch (the body and hand decoders' layers
 * of equal shape): problem g reads x + g*xs_g, weights packed + g*w_gs (each packed by
 * a2m_conv1d_tap_pack_f32), bias / BN arrays at + g*Co, and writes y + g*ys_g (group strides
 * are element offsets of either sign; xs_g may be 0 for a shared input).  Any of
 * bias / BN may be NULL for all problems.  Otherwise as a2m_conv1d_tap_fwd_f32. */
int a2m_conv1d_tap_group_fwd_f32(const float* x, int64_t xs_g, int64_t xs_b, int64_t xs_c, int32_t G,
                                 int32_t B, int32_t Ci, int32_t T, const float* packed, int64_t w_gs,
                                 int32_t chunk, const float* bias, int32_t Co, int32_t ks, int32_t pad,
                                 const float* bn_w, const float* bn_b, const float* bn_rm,
                                 const float* bn_rv, float bn_eps, int32_t act, float slope, float* y,
                                 int64_t ys_g, int64_t ys_b, int64_t ys_c, int64_t ys_t, void* ws,
                                 size_t ws_bytes, void* stream);
/* Winograd F(2,3) form of the 3-tap, pad-1, stride-1 conv1d (opt-in; a2m_conv1d_tap_fwd_f32 is
 * unchanged): two outputs of a clip from 4 multiplies per input channel instead of 6, fp32 only.
 * Weights [Co][Ci][3] are packed once per weight version by a2m_conv1d_wino_pack_f32 as
 * [Co][Ci/32][4][32] (Co*Ci*4 floats): U0 = g0, U1 = (g0+g1+g2)/2, U2 = (g0-g1+g2)/2, U3 = g2.
 * Eligible: fp32 precision, clips of T >= 16 with 64 % T == 0, Ci % 32 == 0, x as for
 * a2m_conv1d_tap_fwd_f32, and a shape the engine's per-shape rule table keeps on the Winograd
 * tile.  The forwards return A2M_EINVAL ("conv1d_wino: not a Winograd launch ...") otherwise;
 * a2m_conv1d_wino_route answers beforehand without launching: out as a2m_gemm_f32_route's, flags
 * bit 4 set where the launch takes the Winograd tile.  With wino = 0 it is the route of the
 * direct tap path (`packed` then stands for the tap-chunked weights), which is also what a
 * refused request gets.  res (may be NULL): a residual added after the activation, addressed
 * like y.  The group entry runs G problems as a2m_conv1d_tap_group_fwd_f32 does (w_gs >=
 * Co*Ci*4).  Epilogue and output strides as a2m_conv1d_fwd_f32. */
int a2m_conv1d_wino_pack_f32(const float* w, int32_t Co, int32_t Ci, float* packed, void* stream);
int a2m_conv1d_wino_route(const float* x, int64_t xs_g, int64_t xs_b, int64_t xs_c, int32_t G, int32_t B,
                          int32_t Ci, int32_t T, const float* packed, int32_t Co, const float* res, float* y,
                          int64_t ys_g, int64_t ys_b, int64_t ys_c, int64_t ys_t, int32_t wino, int32_t out[8]);
int a2m_conv1d_wino_fwd_f32(const float* x, int64_t xs_b, int64_t xs_c, int32_t B, int32_t Ci, int32_t T,
                            const float* packed, const float* bias, int32_t Co, const float* bn_w,
                            const float* bn_b, const float* bn_rm, const float* bn_rv, float bn_eps,
                            int32_t act, float slope, const float* res, float* y, int64_t ys_b, int64_t ys_c,
                            int64_t ys_t, void* ws, size_t ws_bytes, void* stream);
int a2m_conv1d_wino_group_fwd_f32(const float* x, int64_t xs_g, int64_t xs_b, int64_t xs_c, int32_t G,
                                  int32_t B, int32_t Ci, int32_t T, const float* packed, int64_t w_gs,
                                  const float* bias, int32_t Co, const float* bn_w, const float* bn_b,
                                  const float* bn_rm, const float* bn_rv, float bn_eps, int32_t act,
                                  float slope, const float* res, float* y, int64_t ys_g, int64_t ys_b,
                                  int64_t ys_c, int64_t ys_t, void* ws, size_t ws_bytes, void* stream);
/* Toom-Cook F(2,2) form of the 4-tap, stride-2, pad-1 conv1d (opt-in; a2m_conv1d_fwd_f32 is
 * unchanged): no im2col matrix, and two outputs of a clip from 6 multiplies per input channel
 * instead of 8, fp32 only.  The conv is two 2-tap convs over the odd and the even input samples;
 * weights [Co][Ci][4] are packed once per weight version by a2m_conv1d_down_pack_f32 as
 * [Co][Ci/32][6][32] (Co*Ci*6 floats): w0, w2, w1, w3, w0+w2, w1+w3.
 * Eligible: fp32 precision, k = 4, s = 2, p = 1, x t-contiguous with 16-byte aligned rows (xs_b
 * and xs_c multiples of 4), clips of Tin >= 16 with 128 % Tin == 0, Ci % 32 == 0, and a shape the
 * engine's per-shape rule table keeps on this tile.  The forward returns A2M_EINVAL
 * ("conv1d_down: not a down-sampling launch ...") otherwise; a2m_conv1d_down_route answers
 * beforehand without launching: out as a2m_gemm_f32_route's, flags bit 5 set where the launch
 * takes this tile.  With down = 0, and for a refused request, it is the route
 * a2m_conv1d_fwd_f32 takes for the same conv (`w` is inspected for alignment only).  Workspace:
 * split-K slabs only.  Epilogue and output strides as a2m_conv1d_fwd_f32. */
int a2m_conv1d_down_pack_f32(const float* w, int32_t Co, int32_t Ci, float* packed, void* stream);
int a2m_conv1d_down_route(const float* x, int64_t xs_b, int64_t xs_c, int32_t B, int32_t Ci, int32_t Tin,
                          const float* w, int32_t Co, int32_t ks, int32_t stride, int32_t pad, float* y,
                          int64_t ys_b, int64_t ys_c, int64_t ys_t, int32_t down, int32_t out[8]);
int a2m_conv1d_down_fwd_f32(const float* x, int64_t xs_b, int64_t xs_c, int32_t B, int32_t Ci, int32_t Tin,
                            const float* packed, const float* bias, int32_t Co, int32_t ks, int32_t stride,
                            int32_t pad, const float* bn_w, const float* bn_b, const float* bn_rm,
                            const float* bn_rv, float bn_eps, int32_t act, float slope, float* y, int64_t ys_b,
                            int64_t ys_c, int64_t ys_t, void* ws, size_t ws_bytes, void* stream);
/* The same split in two: the per-phase weight packing (packed: Ci*Co*k floats) and the
 * forward on packed weights (callers cache the packing while the weights are unchanged). */
int a2m_convt1d_pack_f32(const float* w, int32_t Ci, int32_t Co, int32_t ks, int32_t stride,
                         int32_t pad, float* packed, void* stream);
int a2m_convt1d_packed_fwd_f32(const float* x, int64_t xs_b, int64_t xs_c, int32_t B, int32_t Ci,
                               int32_t Tin, const float* packed, const float* bias, int32_t Co,
                               int32_t ks, int32_t stride, int32_t pad, int32_t out_pad,
                               const float* bn_w, const float* bn_b, const float* bn_rm,
                               const float* bn_rv, float bn_eps, int32_t act, float slope, float* y,
                               int64_t ys_b, int64_t ys_c, void* ws, size_t ws_bytes, void* stream);
/* The same forward with each phase as a stride-1 tap-chunked conv1d (the GEMM engine's loader
 * mode 5: a channel chunk's x window is loaded once for all of the phase's taps).  Weights
 * packed per phase in `chunk`-channel chunks with reversed taps (chunk = a2m_conv1d_tap_chunk(),
 * Ci % chunk == 0); every phase must hold Tin outputs (Tout = stride * Tin), Tin % 4 == 0 and
 * 64 % Tin == 0, x rows 16-byte aligned.  Replaces nn.ConvTranspose1d.forward at the
 * ConvTranspose1D shapes (model_layers.py:193-215, the UNet up path at :325). */
int a2m_convt1d_tap_pack_f32(const float* w, int32_t Ci, int32_t Co, int32_t ks, int32_t stride,
                             int32_t pad, int32_t chunk, float* packed, void* stream);
int a2m_convt1d_tap_fwd_f32(const float* x, int64_t xs_b, int64_t xs_c, int32_t B, int32_t Ci,
                            int32_t Tin, const float* packed, int32_t chunk, const float* bias,
                            int32_t Co, int32_t ks, int32_t stride, int32_t pad, int32_t out_pad,
                            const float* bn_w, const float* bn_b, const float* bn_rm,
                            const float* bn_rv, float bn_eps, int32_t act, float slope, float* y,
                            int64_t ys_b, int64_t ys_c, void* ws, size_t ws_bytes, void* stream);

/* Channels-last conv2d for the AudioEncoder eval chain (model_layers.py:219-280,
 * ConvNormRelu(type='2d') layers): x NHWC [B][H][W][Ci] (the mel [B][T][F] is already NHWC with
 * Ci = 1), weights packed once by a2m_conv2d_pack_nhwc_f32 as [Co][kh][kw][Ci], output NHWC
 * [B][Hout][Wout][Co] (y_nhwc = 1) or NCHW (0), only columns [w_lo, w_hi) computed.  The GEMM's
 * activation operand is a unit-stride run of kw*Ci floats per (row, kernel row) -- float4 loads,
 * no im2col matrix and no transposed staging.  Requires (kw * Ci) % 4 == 0. */
int a2m_conv2d_pack_nhwc_f32(const float* w, int32_t Co, int32_t Ci, int32_t kh, int32_t kw,
                             float* packed, void* stream);
int a2m_conv2d_nhwc_fwd_f32(const float* x, int32_t B, int32_t Ci, int32_t H, int32_t W,
                            const float* packed, const float* bias, int32_t Co, int32_t kh,
                            int32_t kw, int32_t stride, int32_t pad_h, int32_t pad_w,
                            const float* bn_w, const float* bn_b, const float* bn_rm,
                            const float* bn_rv, float bn_eps, int32_t act, float slope, float* y,
                            int32_t y_nhwc, int32_t Hout, int32_t Wout, int32_t w_lo, int32_t w_hi,
                            void* ws, size_t ws_bytes, void* stream);
/* The AudioEncoder's last ConvNormRelu plus its time resample (model_layers.py:272-279): the
 * channels-last conv of a2m_conv2d_nhwc_fwd_f32 restricted to the one output column w_col that
 * F.interpolate(size=(T,1), mode='bilinear', align_corners=False) reads (it must be that
 * resample's only live column: Wout/2 - 1/2 == w_col, else A2M_EINVAL), with the resample fused
 * into the GEMM's reduce: y [B][Co][T] equals a2m_conv2d_nhwc_fwd_f32 (y_nhwc = 0) followed by
 * a2m_interp_time_f32, bit for bit, without the intermediate tensor or the second launch.
 * Replaces the last conv + interpolate of AudioEncoder.forward (model_layers.py:271-280). */
int a2m_conv2d_nhwc_interp_fwd_f32(const float* x, int32_t B, int32_t Ci, int32_t H, int32_t W,
                                   const float* packed, const float* bias, int32_t Co, int32_t kh,
                                   int32_t kw, int32_t stride, int32_t pad_h, int32_t pad_w,
                                   const float* bn_w, const float* bn_b, const float* bn_rm,
                                   const float* bn_rv, float bn_eps, int32_t act, float slope,
                                   float* y, int32_t T, int32_t Hout, int32_t Wout, int32_t w_col,
                                   void* ws, size_t ws_bytes, void* stream);
/* AudioEncoder's Conv2d ConvNormRelu layers (model_layers.py:219-276) on contiguous
 * [B][Ci][H][W] -> [B][Co][Hout][Wout].  Only output columns [w_lo, w_hi) are computed
 * (the encoder's dead-column pruning); the rest of y is untouched. */
int a2m_conv2d_fwd_f32(const float* x, int32_t B, int32_t Ci, int32_t H, int32_t W,
                       const float* w, const float* bias, int32_t Co, int32_t kh, int32_t kw,
                       int32_t stride, int32_t pad_h, int32_t pad_w,
                       const float* bn_w, const float* bn_b, const float* bn_rm,
                       const float* bn_rv, float bn_eps, int32_t act, float slope,
                       float* y, int32_t Hout, int32_t Wout, int32_t w_lo, int32_t w_hi,
                       void* ws, size_t ws_bytes, void* stream);

/* F.interpolate(x, size=(T,1), mode='bilinear', align_corners=False).squeeze(-1)
 * (model_layers.py:277-279) on x [B][C][H][W] -> y [B][C][T]. */
/* y[b][t][c] = x[b][c][t] (x channel stride T, batch stride xs_b; T <= 64): the [B*T][C]
 * row layout of an activation for GEMMs that want it as dense k-contiguous rows (the UNet's
 * wide attentions do this internally; the decoders' graph-stack input projection,
 * real_motion_model.py:173-176).  No reference counterpart: a layout change. */
int a2m_bct_to_btc_f32(const float* x, int64_t xs_b, int32_t B, int32_t C, int32_t T, float* y,
                       void* stream);
int a2m_interp_time_f32(const float* x, int32_t B, int32_t C, int32_t H, int32_t W,
                        float* y, int32_t T, void* stream);

/* Discriminator plumbing (real_motion_model.py:599,609,620): y[b][c] = scale * mean_t x[b][c][t]
 * and y[b][c][t] = scale * x[b][c] (repeat over time into a strided, e.g. concatenated,
 * buffer).  Each is the other's adjoint up to the scale (used by the backward pass). */
int a2m_mean_time_f32(const float* x, int64_t xs_b, int64_t xs_c, int32_t B, int32_t C,
                      int32_t T, float scale, float* y, void* stream);
int a2m_repeat_time_f32(const float* x, int32_t B, int32_t C, int32_t T, float scale, float* y,
                        int64_t ys_b, int64_t ys_c, void* stream);

/* ---------------------------------------------------------------- attention blocks
 * SelfAttention (model_layers.py:121-146): q,k = 1x1 conv C->C/8, v = 1x1 conv C->C,
 * A = softmax(q^T k) (no 1/sqrt(d) scaling), y = gamma*(v A^T) + x (+ res if not NULL).
 * x, res, y are [B][C][T] with batch stride x_bs / y_bs (res uses y's layout).
 * qkv_out [B][C/4 + C][T] and attn_out [B][T][T] receive the intermediates (kept for the
 * backward pass); ws is split-K scratch. */
int a2m_self_attention_fwd_f32(const float* x, int64_t x_bs, int32_t B, int32_t C, int32_t T,
                               const float* wq, const float* bq, const float* wk,
                               const float* bk, const float* wv, const float* bv,
                               const float* gamma, const float* res,
                               float* y, int64_t y_bs, float* qkv_out, float* attn_out,
                               void* ws, size_t ws_bytes, void* stream);
size_t a2m_self_attention_ws_bytes(int32_t B, int32_t C, int32_t T);
/* The same with the q/k/v 1x1-conv weights pre-stacked by a2m_stack_qkv_f32 into
 * wqkv [C/4 + C][C] and bqkv [C/4 + C] (callers cache these while the weights are unchanged). */
int a2m_stack_qkv_f32(const float* wq, const float* bq, const float* wk, const float* bk,
                      const float* wv, const float* bv, int32_t C, float* wqkv, float* bqkv,
                      void* stream);
int a2m_self_attention_packed_fwd_f32(const float* x, int64_t x_bs, int32_t B, int32_t C,
                                      int32_t T, const float* wqkv, const float* bqkv,
                                      const float* gamma, const float* res, float* y, int64_t y_bs,
                                      float* qkv_out, float* attn_out, void* ws, size_t ws_bytes,
                                      void* stream);
/* Which kernels SelfAttention runs at (C, T), a pure host function: 0 the general path (score
 * GEMM, softmax, PV GEMM), 1 the attention core (C/8 in {16, 32, 48, 64}, T <= 64), 2 the wide
 * core (C/8 in {128, 192, 256}, T <= 32, T % 4 == 0), 3 the fused inference kernel, returned only
 * when keep == 0 (no intermediates wanted) and a2m_self_attention_eval_fits(C, T).
 * a2m_self_attention_packed_fwd_f32 takes its decision from this function with keep = 1. */
int32_t a2m_self_attention_route(int32_t C, int32_t T, int32_t keep);

/* Inference-only SelfAttention with the q/k/v projections fused into the attention core (one
 * launch; no qkv / attention intermediates).  Supported when a2m_self_attention_eval_fits(C, T):
 * C in {128, 256}, 4 <= T <= 64, T % 4 == 0 (the decoders' SelfAttention(256) at T = 64).
 * Same arguments and results as a2m_self_attention_packed_fwd_f32 otherwise. */
int32_t a2m_self_attention_eval_fits(int32_t C, int32_t T);
int a2m_self_attention_eval_f32(const float* x, int64_t x_bs, int32_t B, int32_t C, int32_t T,
                                const float* wqkv, const float* bqkv, const float* gamma,
                                const float* res, float* y, int64_t y_bs, void* stream);
/* The same with wqkv_h, wqkv rounded to bf16 (a2m_to_bf16_f32, 16-byte aligned; made once per
 * weight version), for the bf16 operand mode: the projection stages the ready bf16 weights
 * instead of rounding the fp32 ones in every workgroup -- bitwise the same result.  wqkv_h may
 * be NULL; ignored at precision 0. */
int a2m_self_attention_eval_ex_f32(const float* x, int64_t x_bs, int32_t B, int32_t C, int32_t T,
                                   const float* wqkv, const float* bqkv, const float* gamma,
                                   const float* res, float* y, int64_t y_bs, const void* wqkv_h,
                                   void* stream);

/* G such problems in one launch (grid G*B): problem g has its own wqkv + g*(C/4 + C)*C,
 * bqkv + g*(C/4 + C), gamma + g, and reads x + g*x_gs (batch stride x_bs, also y's), res +
 * g*res_gs, writes y + g*y_gs. */
int a2m_self_attention_eval_group_f32(const float* x, int64_t x_gs, int64_t x_bs, int32_t G, int32_t B,
                                      int32_t C, int32_t T, const float* wqkv, const float* bqkv,
                                      const float* gamma, const float* res, int64_t res_gs, float* y,
                                      int64_t y_gs, void* stream);

/* ChannelAttention (model_layers.py:149-174): y = x * (mlp(avg_T x) + mlp(max_T x)),
 * mlp = Linear(C, C/r) -> ReLU -> Linear(C/r, C) -> Sigmoid.  x, y contiguous [B][C][T];
 * att_out [B][C] (required) receives the channel weights; y may alias x. */
int a2m_channel_attention_fwd_f32(const float* x, int32_t B, int32_t C, int32_t T,
                                  const float* w1, const float* b1, int32_t Cr,
                                  const float* w2, const float* b2,
                                  float* y, float* att_out, void* stream);

/* LayerNorm over the last dim of rows [R][D] (real_motion_model.py:176,207).
 * Output element (r, d) goes to y + (r / T)*ys_b + d*ys_d + (r % T)*ys_t so the decoder's
 * permute(0,2,1) back to [B][C][T] is fused. */
int a2m_layernorm_fwd_f32(const float* x, int32_t R, int32_t D, const float* w, const float* b,
                          float eps, float* y, int32_t T, int64_t ys_b, int64_t ys_d,
                          int64_t ys_t, float* mean_out, float* rstd_out, void* stream);

/* GAT attention projections U[q][k] = sum_c W_h[c][k] att_q[c] (q < 4: att_src of head q,
 * q >= 4: att_dst of head q-4) of one GATConv(64, 64, heads=4): the logits a[n][q] = x_n . U[q]
 * without projecting x.  U: [8][64] device buffer; cache it per weight version. */
int a2m_graph_att_proj_f32(const float* w0, const float* att_src, const float* att_dst, float* U,
                           void* stream);
/* Fused eval graph stack (real_motion_model.py:173-201 body / :225-253 hand, eval mode):
 * nlayers x { y = LeakyReLU(LayerNorm64(L(x))) + x } with L = GATConv(64,64,heads=4,concat=False)
 * (kinds[l] = 0: w0 = lin.weight [256][64], U from a2m_graph_att_proj_f32, bias) or GraphConv
 * (kinds[l] = 1: w0 = lin_rel.weight, w1 = lin_root.weight, bias = lin_rel.bias).  The
 * per-layer arrays are host arrays of device pointers.  One launch; each workgroup keeps its
 * frames' node tile in LDS across the layers.  x, y: [F*J][64], distinct.
 * Topology limits (nbr_ptr / nbr_idx are device arrays, so they are NOT checked here; the
 * Python host side validates them where the CSR is built, a2m/skeleton.py in_neighbour_csr):
 * J <= 128, in-degree <= 7 per node, and (J + 1) + nbr_ptr[J] <= 256.  A topology beyond
 * them gives wrong results. */
int a2m_graph_stack_fwd_f32(const float* x, int32_t F, int32_t J, const int32_t* nbr_ptr,
                            const int32_t* nbr_idx, int32_t nlayers, const int32_t* kinds,
                            const float* const* w0, const float* const* w1, const float* const* U,
                            const float* const* bias, const float* const* ln_w,
                            const float* const* ln_b, float slope, float* y, void* stream);
/* The same with bf16 copies of the layer weights for the bf16 operand mode (precision 1):
 * w0h[l] / w1h[l] are device buffers holding w0[l] / w1[l] rounded to bf16 (a2m_to_bf16_f32, same
 * [row][64] layout, 16-byte aligned), made once per weight version, so the layers' k loops load
 * ready bf16 fragments instead of rounding the fp32 weights each time (the same values: the
 * result is bitwise that of a2m_graph_stack_fwd_f32).  w0h / w1h (the arrays or a layer's
 * entries) may be NULL; ignored at precision 0. */
int a2m_graph_stack_fwd_ex_f32(const float* x, int32_t F, int32_t J, const int32_t* nbr_ptr,
                               const int32_t* nbr_idx, int32_t nlayers, const int32_t* kinds,
                               const float* const* w0, const float* const* w1, const float* const* U,
                               const float* const* bias, const float* const* ln_w,
                               const float* const* ln_b, const void* const* w0h,
                               const void* const* w1h, float slope, float* y, void* stream);
/* The stack's topology plan: the degree-sorted row order, the in-degrees and the gather slots of
 * one full workgroup tile (128 / J frames), which depend on the skeleton alone.  Built on the HOST
 * from the in-neighbour CSR as host arrays -- no device call -- and copied to device memory once by
 * the caller, like the a2m_logmel_* plan.  a2m_graph_stack_plan_build checks the topology limits
 * above and returns A2M_EINVAL beyond them; a2m_graph_stack_plan_bytes returns 0 then.
 * Layout: 128 rows of 12 bytes in sorted-row order (in-degree descending, node index ascending
 * within a degree): node, in-degree d, 8 gather slots (the in-neighbours in edge order as
 * tile-local node indices f * J + source, the node itself at slot d, 0 after), 2 bytes of
 * padding; rows past the tile's (128 / J) * J nodes carry node 0xff. */
size_t a2m_graph_stack_plan_bytes(int32_t J, const int32_t* nbr_ptr, const int32_t* nbr_idx);
int a2m_graph_stack_plan_build(int32_t J, const int32_t* nbr_ptr, const int32_t* nbr_idx,
                               void* host_plan, size_t plan_bytes);
/* a2m_graph_stack_fwd_ex_f32 with the plan (device memory, 4-byte aligned, built for this J and
 * CSR): the workgroups read their rows from it instead of rebuilding the tables in LDS.  The
 * result is that of plan = NULL, which is a2m_graph_stack_fwd_ex_f32. */
int a2m_graph_stack_fwd_ex2_f32(const float* x, int32_t F, int32_t J, const int32_t* nbr_ptr,
                                const int32_t* nbr_idx, int32_t nlayers, const int32_t* kinds,
                                const float* const* w0, const float* const* w1, const float* const* U,
                                const float* const* bias, const float* const* ln_w,
                                const float* const* ln_b, const void* const* w0h,
                                const void* const* w1h, const void* plan, float slope, float* y,
                                void* stream);
/* y[i] = bf16(x[i]), round to nearest even (the rounding the bf16 operand mode applies), n
 * elements; y 4-byte aligned, 2 bytes an element. */
int a2m_to_bf16_f32(const float* x, void* y, int64_t n, void* stream);
/* ---------------------------------------------------------------- skeleton graph layers
 * One fused GNN step of the body / hand decoders (real_motion_model.py:173-201, 225-253):
 *   y = LeakyReLU(LayerNorm64(L(x))) + x
 * for every frame's J-node skeleton graph (nodes [F][J][64] contiguous), where L is
 *   kind 0: GATConv(64,64,heads=4,concat=False) + self loops; wlin [256][64], att_src,
 *           att_dst [4][64], bias [64]
 *   kind 1: GraphConv(64,64): W_rel (sum_nbr x) + b_rel + W_root x
 * The topology is given as an in-neighbour CSR over one graph (nbr_ptr[J+1], nbr_idx,
 * source nodes of the edges into each target, in edge order) and is shared by all F
 * frames (limits as for a2m_graph_stack_fwd_f32: J <= 128, in-degree <= 7,
 * (J + 1) + nbr_ptr[J] <= 256; not checked on the device arrays).  A topology without an edge
 * (nbr_ptr all zero) may pass nbr_idx = NULL, here and to the layer backward.  norm_res = 0 gives the bare layer y = L(x) (the discriminator's per-sample
 * GATConv, real_motion_model.py:602-616).  lin_out (GAT: x' [F*J][256]; GraphConv: aggregated x [F*J][64]) and
 * pre_ln [F*J][64] are saved for the backward pass when not NULL. */
int a2m_graph_layer_fwd_f32(const float* x, int32_t F, int32_t J, int32_t kind,
                            int32_t norm_res, const int32_t* nbr_ptr, const int32_t* nbr_idx,
                            const float* w0, const float* w1, const float* att_src,
                            const float* att_dst, const float* bias,
                            const float* ln_w, const float* ln_b, float slope,
                            float* y, float* lin_out, float* pre_ln,
                            void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- pose losses
 * compute_bone_length_loss (real_motion_model.py:307-347) and
 * compute_comprehensive_angle_loss (:449-461, hand :350-392, body :394-447) on interleaved
 * (x, y) poses [B][T][104] with element (b,t,f) at p + b*ps_b + t*ps_t + f.
 * out[0] = bone loss (0 if real == NULL), out[1] = 0.7*hand + 0.3*body angle loss. */
int a2m_pose_losses_f32(const float* gen, int64_t gs_b, int64_t gs_t, const float* real,
                        int64_t rs_b, int64_t rs_t, int32_t B, int32_t T, float* out,
                        void* ws, size_t ws_bytes, void* stream);
/* The same with the angle weights explicit: out[1] = hand_w * hand + body_w * body.
 * (1, 0) is compute_hand_joint_angle_loss (real_motion_model.py:350-392), (0, 1)
 * compute_body_joint_angle_loss (:394-447), (0.7, 0.3) the comprehensive loss (:449-461). */
int a2m_pose_losses_w_f32(const float* gen, int64_t gs_b, int64_t gs_t, const float* real,
                          int64_t rs_b, int64_t rs_t, int32_t B, int32_t T, float hand_w,
                          float body_w, float* out, void* ws, size_t ws_bytes, void* stream);

/* ================================================================ training step
 * Forward-in-train-mode and backward entry points for the per-clip GAN step
 * (version5_model_train.py:342-405).  Gradients are written (accumulate = 0) or added
 * (accumulate = 1) into caller buffers; reductions are done in a fixed order. */

/* BatchNorm in training mode (nn.BatchNorm1d/2d forward with batch statistics, running
 * stats updated in place with `momentum`, unbiased running variance) fused with dropout
 * and the activation.  x is the raw conv output, element (b, c, l) at b*xs_b + c*xs_c + l.
 * drop_mode: 0 none, 1 element dropout before BN (ConvNormRelu 1-d, model_layers.py:118),
 * 2 channel dropout before BN (Dropout2d, 2-d ConvNormRelu), 3 element dropout after the
 * activation (discriminator blocks, real_motion_model.py:504-551).  Masks are a hash of
 * (seed, element index) and are regenerated by the backward pass.  drop_p outside [0, 1) or an
 * unknown drop_mode is A2M_EINVAL in every a2m_bn_* entry (p = 1 has no keep-scale).  Limit: B * L < 2^31
 * elements per channel (32-bit slice indexing; A2M_EINVAL beyond -- such a channel alone
 * would be 8 GB, more than any tensor of this model at any batch that fits one GPU). */
int a2m_bn_train_fwd_f32(const float* x, int64_t xs_b, int64_t xs_c, int32_t B, int32_t C,
                         int32_t L, const float* gamma, const float* beta, float* running_mean,
                         float* running_var, float momentum, float eps, float drop_p,
                         int32_t drop_mode, uint64_t seed, int32_t act, float slope, float* y,
                         int64_t ys_b, int64_t ys_c, float* save_mean, float* save_rstd,
                         void* ws, size_t ws_bytes, void* stream);
/* dx (contiguous [B][C][L]) = d(loss)/d(raw conv output); dbias = sum over (b, l) of dx. */
int a2m_bn_train_bwd_f32(const float* dy, int64_t dys_b, int64_t dys_c, const float* x,
                         int64_t xs_b, int64_t xs_c, int32_t B, int32_t C, int32_t L,
                         const float* gamma, const float* beta, const float* save_mean,
                         const float* save_rstd, float drop_p, int32_t drop_mode, uint64_t seed,
                         int32_t act, float slope, float* dx, float* dgamma, float* dbeta,
                         float* dbias, void* ws, size_t ws_bytes, void* stream);
/* Eval-mode BatchNorm with gradients (nn.BatchNorm*d after .eval(), model_layers.py:51-118, e.g.
 * fine-tuning or input attribution through a frozen G): normalises with the running statistics,
 * which it does not update, fused with the activation; save_mean / save_rstd receive the running
 * mean and 1 / sqrt(running_var + eps) for the backward.  drop_p / drop_mode / seed as in
 * a2m_bn_train_fwd_f32: the surrounding Dropout module may still be in training mode when only the
 * norm is frozen (bn.eval(), dropout left on); pass drop_p = 0 for a whole module in eval. */
int a2m_bn_eval_fwd_f32(const float* x, int64_t xs_b, int64_t xs_c, int32_t B, int32_t C, int32_t L,
                        const float* gamma, const float* beta, const float* running_mean,
                        const float* running_var, float eps, float drop_p, int32_t drop_mode,
                        uint64_t seed, int32_t act, float slope, float* y, int64_t ys_b, int64_t ys_c,
                        float* save_mean, float* save_rstd, void* stream);
/* Its backward: dx = gamma * rstd * act'(.) * dy (* the dropout scale; fixed statistics: no
 * batch-mean terms), dgamma = sum g * xhat, dbeta = sum g, dbias = sum dx, g = act'(.) * dy. */
int a2m_bn_eval_bwd_f32(const float* dy, int64_t dys_b, int64_t dys_c, const float* x, int64_t xs_b,
                        int64_t xs_c, int32_t B, int32_t C, int32_t L, const float* gamma,
                        const float* beta, const float* save_mean, const float* save_rstd, float drop_p,
                        int32_t drop_mode, uint64_t seed, int32_t act, float slope, float* dx,
                        float* dgamma, float* dbeta, float* dbias, void* ws, size_t ws_bytes,
                        void* stream);
/* Dropout seed offset for training steps captured in a HIP graph (version5_model_train.py:
 * 342-405 replayed per G / D step): every dropout launch issued while `counter` (a device
 * uint64) is registered hashes with seed + counter[0] * K, read when the kernel runs, so a
 * replayed step that advances the counter draws fresh masks although its seeds are baked.
 * NULL (the default) restores the plain seeds.  Library-global; set it around the launches. */
int a2m_set_dropout_seed_offset(const uint64_t* counter);
/* SyncBatchNorm phases for data-parallel training (per-layer all-reduce of the
 * BatchNorm statistics so DP over ranks normalises like the single-device batch,
 * version5_model_train.py:342-414 at B = 64).  The fused bn_train_fwd/bwd above split at their
 * per-channel reductions; the caller all-reduces (SUM) the float64 pairs between the phases:
 *   fwd:  sync_stats -> sums[C][2] = (sum z, sum z^2) -> all-reduce -> sync_apply(n_total)
 *   bwd:  sync_bwd_stats -> sums[C][2] = (sum g, sum g*xhat), local dbeta / dgamma
 *         -> all-reduce -> sync_bwd_apply(n_total).   n_total = sum over ranks of B*L. */
int a2m_bn_sync_stats_f32(const float* x, int64_t xs_b, int64_t xs_c, int32_t B, int32_t C,
                          int32_t L, float drop_p, int32_t drop_mode, uint64_t seed, double* sums,
                          void* ws, size_t ws_bytes, void* stream);
int a2m_bn_sync_apply_f32(const float* x, int64_t xs_b, int64_t xs_c, int32_t B, int32_t C,
                          int32_t L, const double* sums, int64_t n_total, const float* gamma,
                          const float* beta, float* running_mean, float* running_var,
                          float momentum, float eps, float drop_p, int32_t drop_mode,
                          uint64_t seed, int32_t act, float slope, float* y, int64_t ys_b,
                          int64_t ys_c, float* save_mean, float* save_rstd, void* stream);
int a2m_bn_sync_bwd_stats_f32(const float* dy, int64_t dys_b, int64_t dys_c, const float* x,
                              int64_t xs_b, int64_t xs_c, int32_t B, int32_t C, int32_t L,
                              const float* gamma, const float* beta, const float* save_mean,
                              const float* save_rstd, float drop_p, int32_t drop_mode,
                              uint64_t seed, int32_t act, float slope, double* sums,
                              float* dgamma, float* dbeta, void* ws, size_t ws_bytes, void* stream);
int a2m_bn_sync_bwd_apply_f32(const float* dy, int64_t dys_b, int64_t dys_c, const float* x,
                              int64_t xs_b, int64_t xs_c, int32_t B, int32_t C, int32_t L,
                              const float* gamma, const float* beta, const float* save_mean,
                              const float* save_rstd, float drop_p, int32_t drop_mode,
                              uint64_t seed, int32_t act, float slope, const double* sums,
                              int64_t n_total, float* dx, float* dbias, void* ws, size_t ws_bytes,
                              void* stream);
/* nn.Dropout(p) with the hash mask (real_motion_model.py:203,255); backward = same call. */
int a2m_dropout_f32(const float* x, int64_t n, float p, uint64_t seed, float* y, void* stream);
/* y[c] (+)= sum_{b,t} x[b][c][t] (conv / linear bias gradients). */
int a2m_sum_bt_f32(const float* x, int64_t xs_b, int64_t xs_c, int64_t xs_t, int32_t B,
                   int32_t C, int32_t T, float* y, int32_t accumulate, void* stream);
/* LayerNorm backward; dy in the same (permuted) layout the forward wrote. */
int a2m_layernorm_bwd_f32(const float* dy, int64_t dys_b, int64_t dys_d, int64_t dys_t,
                          int32_t T, const float* x, int32_t R, int32_t D, const float* w,
                          const float* mean, const float* rstd, float* dx, float* dw, float* db,
                          void* ws, size_t ws_bytes, void* stream);

/* Conv2d / Conv1d (H = kh = 1) backward.  dgrad: dy contiguous [B][Co][Ho][Wo] ->
 * dx (strided) by output-phase decomposed implicit GEMMs (also ConvTranspose1d's forward
 * algebra); wgrad: dw [Co][Ci][kh][kw] = sum dy (x) im2col(x). */
int a2m_conv2d_dgrad_f32(const float* dy, int32_t B, int32_t Co, int32_t Ho, int32_t Wo,
                         const float* w, int32_t Ci, int32_t H, int32_t W, int32_t kh, int32_t kw,
                         int32_t stride_h, int32_t stride_w, int32_t pad_h, int32_t pad_w,
                         float* dx, int64_t dxs_b, int64_t dxs_c, int64_t dxs_h, int64_t dxs_w,
                         int32_t accumulate, void* ws, size_t ws_bytes, void* stream);
int a2m_conv2d_wgrad_f32(const float* dy, int32_t B, int32_t Co, int32_t Ho, int32_t Wo,
                         const float* x, int64_t xs_b, int64_t xs_c, int64_t xs_h, int64_t xs_w,
                         int32_t Ci, int32_t H, int32_t W, int32_t kh, int32_t kw,
                         int32_t stride_h, int32_t stride_w, int32_t pad_h, int32_t pad_w,
                         float* dw, int32_t accumulate, void* ws, size_t ws_bytes, void* stream);

/* SelfAttention / ChannelAttention backward (inputs: the forward's saved qkv / attention). */
size_t a2m_self_attention_bwd_ws_bytes(int32_t B, int32_t C, int32_t T);
int a2m_self_attention_bwd_f32(const float* dy, const float* x, int64_t bs, int32_t B, int32_t C,
                               int32_t T, const float* wq, const float* bq, const float* wk,
                               const float* bk, const float* wv, const float* bv,
                               const float* gamma, const float* qkv, const float* attn, float* dx,
                               float* dwq, float* dbq, float* dwk, float* dbk, float* dwv,
                               float* dbv, float* dgamma, void* ws, size_t ws_bytes, void* stream);
int a2m_channel_attention_bwd_f32(const float* dy, const float* x, int32_t B, int32_t C, int32_t T,
                                  const float* w1, const float* b1, int32_t Cr, const float* w2,
                                  const float* b2, float* dx, float* dw1, float* db1, float* dw2,
                                  float* db2, void* ws, size_t ws_bytes, void* stream);

/* Skeleton graph layer backward (recomputes the forward from x).
   The topology must be symmetric: every edge j->i of the in-neighbour CSR has its reverse i->j,
   as many times as it occurs itself.  The kernel gathers dx, the source-logit gradients and the
   saved path's aggregation adjoint over a node's in-neighbours, where the adjoint sums over its
   out-neighbours; on a directed topology these are wrong and no error is raised.  A directed
   topology is valid for the forward entries only (a2m_graph_layer_fwd_f32, a2m_graph_stack_*).
   skeleton.in_neighbour_csr(..., symmetric=True) checks the requirement. */
int a2m_graph_layer_bwd_f32(const float* x, const float* dy, int32_t F, int32_t J, int32_t kind,
                            int32_t norm_res, const int32_t* nbr_ptr, const int32_t* nbr_idx,
                            const float* w0, const float* w1, const float* att_src,
                            const float* att_dst, const float* bias, const float* ln_w,
                            const float* ln_b, float slope, float* dx, float* dw0, float* dw1,
                            float* datt_src, float* datt_dst, float* dbias, float* dln_w,
                            float* dln_b, void* ws, size_t ws_bytes, void* stream);
/* The same with the forward's saved pre-LayerNorm output (a2m_graph_layer_fwd_f32's pre_ln,
   norm_res layers; NULL = recompute): no forward recompute in the backward kernel, and the
   weight gradients contract the aggregation adjoint of dout with x (same sums, another order).
   The same symmetric-topology requirement as a2m_graph_layer_bwd_f32. */
int a2m_graph_layer_bwd_saved_f32(const float* x, const float* dy, const float* pre_ln, int32_t F,
                                  int32_t J, int32_t kind, int32_t norm_res, const int32_t* nbr_ptr,
                                  const int32_t* nbr_idx, const float* w0, const float* w1,
                                  const float* att_src, const float* att_dst, const float* bias,
                                  const float* ln_w, const float* ln_b, float slope, float* dx,
                                  float* dw0, float* dw1, float* datt_src, float* datt_dst, float* dbias,
                                  float* dln_w, float* dln_b, void* ws, size_t ws_bytes, void* stream);

/* F.interpolate (time) backward: dx [B][C][H][W] (zeros where the forward read nothing). */
int a2m_interp_time_bwd_f32(const float* dy, int32_t B, int32_t C, int32_t H, int32_t W,
                            float* dx, int32_t T, void* stream);

/* Losses of the G / D steps (version5_model_train.py:208-248, 367-403).
 * The pose-loss backward ADDS grad_out[0] d bone / d gen + grad_out[1] d angle / d gen into dgen
 * ([B][T][104] contiguous): the caller zeroes dgen first, or passes a gradient to add to.  With
 * real == NULL there is no bone term (grad_out[0] is not used). */
int a2m_pose_losses_bwd_f32(const float* gen, int64_t gs_b, int64_t gs_t, const float* real,
                            int64_t rs_b, int64_t rs_t, int32_t B, int32_t T,
                            const float* grad_out, float* dgen, void* ws, size_t ws_bytes,
                            void* stream);
int a2m_pose_losses_w_bwd_f32(const float* gen, int64_t gs_b, int64_t gs_t, const float* real,
                              int64_t rs_b, int64_t rs_t, int32_t B, int32_t T, float hand_w,
                              float body_w, const float* grad_out, float* dgen, void* ws,
                              size_t ws_bytes, void* stream);
/* terms = [L1(diff(real), diff(fake)), mean||accel||, mean||jerk||] on [B][T][Fd] (contiguous).
 * 2 <= T <= 512.  A term over no frames is 0, not the NaN of an empty mean: terms[1] = 0 at
 * T = 2 and terms[2] = 0 at T <= 3, and such a term adds nothing to dfake; terms[0] = 0 and has
 * no gradient if real == NULL.
 * grad_terms (device [3], the incoming dL/dterms) and dfake come together: with both,
 * dfake = sum_i grad_terms[i] * dterms[i]/dfake (overwritten; 0 through a zero norm or a zero
 * L1 difference, as torch); with neither, only the terms; one without the other is A2M_EINVAL. */
int a2m_motion_losses_f32(const float* fake, const float* real, int32_t B, int32_t T, int32_t Fd,
                          float* terms, const float* grad_terms, float* dfake, void* ws,
                          size_t ws_bytes, void* stream);
/* loss = mean (pred - target)^2; dpred (optional) = grad_loss[0] * 2 (pred - target) / n
 * (grad_loss: device scalar, NULL = 1). */
int a2m_mse_loss_f32(const float* pred, const float* target, int64_t n, float* loss,
                     const float* grad_loss, float* dpred, void* ws, size_t ws_bytes, void* stream);
/* pos_to_motion (version5_model_train.py:208): y[b][t] = x[b][t+1] - x[b][t], and its adjoint. */
int a2m_diff_time_f32(const float* x, int32_t B, int32_t T, int32_t Fd, float* y, void* stream);
int a2m_diff_time_bwd_f32(const float* dy, int32_t B, int32_t T, int32_t Fd, float* dx,
                          int32_t accumulate, void* stream);

/* The validation pass of one dev batch (version5_model_train.py:438-480) in two launches around a
 * single discriminator forward.
 * a2m_val_motion_f32: fake_pose, real_pose [B][T][Fd] contiguous.  motion [2B][T-1][Fd]: rows
 * 0..B-1 = diff_t(fake_pose), rows B..2B-1 = diff_t(real_pose), each the one float32 subtraction
 * of a2m_diff_time_f32.  part [B][3] (float64, the caller's own buffer, not the workspace: D's
 * GEMMs use that between the two launches): per clip the sums of |diff(real) - diff(fake)|, of
 * the acceleration norms over t < T-2 and of the jerk norms over t < T-3, the norms in float32 as
 * a2m_motion_losses_f32 takes them, the sums in float64.  One workgroup per clip; every pose
 * element is loaded once.  T >= 2 (no upper bound), Fd <= 1920, T * Fd < 2^31.
 * a2m_val_finish_f32: logits [2B][L] = D's output on `motion` (fake rows first); bone, angle:
 * device scalars (the generator's internal losses).  One workgroup adds to acc [8] (float64,
 * never overwritten: zero it once per epoch)
 *   motion_l1 + lambda_gan * mean((fake_logits - 1)^2),
 *   mean((real_logits - 1)^2) + lambda_d * mean(fake_logits^2),
 *   bone, angle, smoothness, jerk, motion_l1, 1
 * with motion_l1 = sum / (B (T-1) Fd), smoothness = sum / (B (T-2)), jerk = sum / (B (T-3)); a
 * term over no frames is 0 (smoothness at T = 2, jerk at T <= 3).  All sums run in float64 in a
 * fixed order, with no atomics: the same inputs give the same bits on every run. */
int a2m_val_motion_f32(const float* fake_pose, const float* real_pose, int32_t B, int32_t T, int32_t Fd,
                       float* motion, double* part, void* stream);
int a2m_val_finish_f32(const double* part, int32_t B, int32_t T, int32_t Fd, const float* logits,
                       int32_t L, const float* bone, const float* angle, float lambda_gan,
                       float lambda_d, double* acc, void* stream);

/* The evaluation pass over one batch of a split (a2m.evaluation.PoseEvaluator) in
 * three launches.  Poses are [B][T][F] contiguous, a frame being its x row then its y row of
 * K = F / 2 keypoints; style [B] (int32) names each clip's accumulators, and a clip whose style is
 * outside [0, n_styles) is left out of every metric and counted as dropped.  Every floating-point
 * sum runs in float64 in a fixed order with no atomics; only the integer histogram counters are
 * updated with atomicAdd.  The accumulators are never overwritten: zero them once per pass.
 * a2m_eval_clip_f32: fake_px = fake_norm * std + mean (two float32 roundings, as
 * a2m_pose_denormalize_f32; written for every clip).  Per counted clip: hits [B] = the keypoints of
 * all frames within alpha * max(x extent, y extent) of the real frame (float64 on the float32
 * coordinates, <=, as a2m_pck_f32); part [B][3] (float64) = the sums of |fake_px - real_px|, of the
 * real and of the generated speeds.  The speed of frame t >= 1 is the mean over joints 1..K-1 of
 * |p[t] - p[t-1]|, the acceleration of t >= 2 that of |p[t] - 2 p[t-1] + p[t-2]|, in float64; each
 * is counted in bin min(floor(v / width), n_bins - 1) of hist [n_styles][4][n_bins] (int64; real
 * speed, generated speed, real acceleration, generated acceleration).  One workgroup per clip;
 * T >= 1 (no upper bound), F even, 4 <= F <= 2560, T * F < 2^31.
 * a2m_eval_gram_f64: adds to sx [n_styles][2][F] and gram [n_styles][2][F][F] (float64; real, then
 * generated) the sums of x and of x x^T over the frames of each style's clips, float64 products and
 * sums on the MFMA unit.  Only the 16 x 16 tiles on and above the diagonal are written
 * (gram[i][j] with i / 16 <= j / 16); the rest is the mirror image.  Each tile has one owning wave,
 * which takes the clips in ascending order and a clip's frames in ascending steps of 4.
 * a2m_eval_finish_f64: adds the clips' partials, clips ascending, to counts [3 n_styles + 1]
 * (int64; per style clips, frames, hits, then the dropped clips) and sums [n_styles][3] (float64;
 * per style L1, real speed, generated speed).  One wave. */
int a2m_eval_clip_f32(const float* fake_norm, const float* real_px, const int32_t* style, const float* mean,
                      const float* std_, int32_t B, int32_t T, int32_t F, int32_t n_styles, double alpha,
                      int32_t n_bins, double speed_width, double accel_width, float* fake_px, double* part,
                      int32_t* hits, int64_t* hist, void* stream);
int a2m_eval_gram_f64(const float* fake_px, const float* real_px, const int32_t* style, int32_t B, int32_t T,
                      int32_t F, int32_t n_styles, double* sx, double* gram, void* stream);
int a2m_eval_finish_f64(const double* part, const int32_t* hits, const int32_t* style, int32_t B, int32_t T,
                        int32_t n_styles, int64_t* counts, double* sums, void* stream);

/* The audio-motion synchrony metrics of the same pass (a2m.evaluation.AudioSyncEvaluator; DESIGN.md
 * 7.7), two launches a batch, opt-in.  audio [B][T][C] is the audio feature as the generator got
 * it, audio_std [C] its standardisation's std or null (then 1); fake_px, real_px [B][T][F] and
 * style [B] as above.  All arithmetic is float64 on the float32 inputs, every floating-point sum in
 * a fixed order with no atomics; the integer counters are updated with atomicAdd.  A clip whose
 * style is outside [0, n_styles) adds to no accumulator.  The accumulators are added to: zero them
 * once per pass.
 * a2m_eval_sync_f64, per clip and for t = 1..T-1:
 *   onset o[t] = (1 / C) sum_c max(0, (audio[t][c] - audio[t-1][c]) * audio_std[c]),
 *   speed s[t] as a2m_eval_clip_f32's, of the real and of the generated pose;
 *   an audio beat at t in [2, T-2] where o[t] > o[t-1], o[t] >= o[t+1] and o[t] > onset_delta times the
 *   clip's mean of o[1..T-1]; a motion beat where s[t] < s[t-1] and s[t] <= s[t+1].
 *   beat_dist [n_styles][2][2][n_dist] (int64; real | generated pose, motion->audio | audio->motion)
 *   counts every beat's distance in frames to the clip's nearest beat of the other kind in bin
 *   min(d, n_dist - 1), the last bin also where there is none; beat_counts [n_styles][3] (int64) the
 *   audio, real motion and generated motion beats.  part [B][2 n_lags + 1][8] (float64, written for
 *   counted clips only): for the lag l = index - n_lags, over the pairs (o[t], s[t+l]) with t and t + l
 *   in [1, T-1], the sums of o, o^2, then of s, s^2, o s for the real and again for the generated pose.
 *   onset_out [B][T] and speed_out [B][2][T] (float64, real then generated, entry 0 zero; either may
 *   be null) get the series of every clip.  One workgroup per clip, its series in LDS (25 B a
 *   frame: three doubles and a flag byte, 51,200 B at the bound): T <= 2048;
 *   F even and >= 4, n_dist >= 2, 0 <= n_lags <= 16, onset_delta finite and >= 0.
 * a2m_eval_sync_finish_f64: adds part, clips ascending, per style to lag_sums
 *   [n_styles][2 n_lags + 1][8] (float64), and to lag_n [n_styles][2 n_lags + 1] (int64) the number
 *   of pairs, max(T - 1 - |l|, 0) per counted clip.  One wave.  It loads every clip's row of part,
 *   the unwritten rows of dropped clips too, and discards those by a select: part must be B rows of
 *   readable memory, whatever the dropped rows hold. */
int a2m_eval_sync_f64(const float* audio, const float* fake_px, const float* real_px, const int32_t* style,
                      const float* audio_std, int32_t B, int32_t T, int32_t C, int32_t F, int32_t n_styles,
                      int32_t n_lags, int32_t n_dist, double onset_delta, int64_t* beat_dist, int64_t* beat_counts,
                      double* part, double* onset_out, double* speed_out, void* stream);
int a2m_eval_sync_finish_f64(const double* part, const int32_t* style, int32_t B, int32_t T, int32_t n_styles,
                             int32_t n_lags, double* lag_sums, int64_t* lag_n, void* stream);

/* General strided GEMM on the same MFMA engine (linear layers' backward, 1x1 projections):
 *   C[m][n] (+)= alpha * sum_k A(m,k) B(n,k) (+ bias[m]), per batch z < batch
 *   n = n0*N1 + n1, k = k0*K1 + k1 (two-level index spaces cover [B][C][T] row sets)
 *   A(m,k) = A[z*a_bs + m*a_m + k0*a_k0 + k1*a_k1]
 *   B(n,k) = B[z*b_bs + n0*b_n0 + n1*b_n1 + k0*b_k0 + k1*b_k1]
 *   C(m,n) = C[z*c_bs + m*c_m + n0*c_n0 + n1*c_n1]                                        */
int a2m_gemm_f32(int32_t M, int32_t N, int32_t N1, int32_t K, int32_t K1, int32_t batch,
                 const float* A, int64_t a_bs, int64_t a_m, int64_t a_k0, int64_t a_k1,
                 const float* B, int64_t b_bs, int64_t b_n0, int64_t b_n1, int64_t b_k0,
                 int64_t b_k1, float* C, int64_t c_bs, int64_t c_m, int64_t c_n0, int64_t c_n1,
                 const float* bias, float alpha, int32_t accumulate, void* ws, size_t ws_bytes,
                 void* stream);

/* Which tile kernel an engine launch runs: gemm_tile with one wave group per 64x64 / 128x128 tile,
 * gemm_tile with two wave groups (fp32 dense 64x64), the software-pipelined 64x64 tile (fp32 or
 * bf16 operands), or the paired launch of two ConvTranspose1d phases on the pipelined tile. */
#define A2M_GEMM_KIND_TILE 0
#define A2M_GEMM_KIND_TILE_KS2 1
#define A2M_GEMM_KIND_PIPE 2
#define A2M_GEMM_KIND_PIPE_PAIR 3
/* The launch decision a2m_gemm_f32 would take for these arguments under the current precision
 * and overrides, without launching: out = {kind (A2M_GEMM_KIND_*), tile, k-tile depth, split-K
 * count, k per split, A operand mode, B operand mode, flags}; flags bit 0: float4 output rows,
 * bit 1: m-contiguous output, bit 2: halo layout, bit 3: a split-K reduce kernel follows.
 * The pointers are inspected for alignment only and never dereferenced; no GPU is needed. */
int a2m_gemm_f32_route(int32_t M, int32_t N, int32_t N1, int32_t K, int32_t K1, int32_t batch,
                       const float* A, int64_t a_bs, int64_t a_m, int64_t a_k0, int64_t a_k1,
                       const float* B, int64_t b_bs, int64_t b_n0, int64_t b_n1, int64_t b_k0,
                       int64_t b_k1, float* C, int64_t c_bs, int64_t c_m, int64_t c_n0, int64_t c_n1,
                       const float* bias, float alpha, int32_t accumulate, int32_t out[8]);
/* Engine launches per kind (counts[A2M_GEMM_KIND_*]) since the last reset; a paired launch counts
 * once, a launch captured into a graph counts at capture.  reset != 0 zeroes the counters. */
int a2m_gemm_kernel_counts(int64_t counts[4], int32_t reset);

/* torch.optim.Adam step (no weight decay by default, no amsgrad) over a flat buffer. */
int a2m_adam_f32(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                 float lr, float beta1, float beta2, float eps, float weight_decay, int32_t step,
                 void* stream);

/* The same update for a step captured in a HIP graph: step (device int32) is advanced by one in
 * the launch and the bias corrections derived from it on the device; lr is a device float the
 * host rewrites when DynamicGANTraining changes it (version5_model_train.py:80-107).  Bitwise
 * the update of a2m_adam_f32 at the same step and lr. */
int a2m_adam_dev_f32(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                     const float* lr, float beta1, float beta2, float eps, float weight_decay,
                     int32_t* step, void* stream);

/* dst[dst_off[i] .. dst_off[i] + n[i]) = src[i][0 .. n[i]) for i < count (host arrays of device
 * pointers / element counts; segments must not overlap; src[i] may be NULL where n[i] = 0).
 * The optimiser's gradient collection:
 * per-parameter gradient tensors into the flat gradient buffer, 48 segments per launch.
 * Replaces torch's per-parameter AccumulateGrad add (version5_model_train.py:285-286 Adam over
 * model.parameters()). */
int a2m_gather_segments_f32(const float* const* src, const int64_t* dst_off, const int64_t* n,
                            int32_t count, float* dst, void* stream);

/* ---- Pose normalisation and evaluation ----
 * Poses are [n_frames][104] planar (x of 52 joints, then y), neck = joint 0.
 * a2m_pose_moments_f32: acc[0:104] += mean over the frames of (x - neck) (necksub = 1) or x,
 * acc[104:208] += mean of squares, fp64 -- one batch of normalization_tools.get_mean_std[_necksub]
 * (normalization_tools.py:7-45); the caller averages over batches.
 * a2m_pose_normalize_f32: ((x - neck) - mean) / std  (version5_model_train.py:298-304).
 * a2m_pose_denormalize_f32: x * std + mean  (generate_motion_video.py:259-260).
 * a2m_pck_f32: pred, gt [N][2][K] -> out[N] = fraction of keypoints with
 * |gt - pred| <= alpha * max(x extent, y extent) of gt (motion_evaluation.py:4-22).
 * normalize / denormalize with n_frames = 0 and pck with N = 0 do nothing and accept NULL data
 * pointers (an empty batch has none). */
int a2m_pose_moments_f32(const float* pose, int64_t n_frames, int32_t necksub, double* acc,
                         void* stream);
int a2m_pose_normalize_f32(const float* pose, int64_t n_frames, const float* mean, const float* std_,
                           float* out, void* stream);
int a2m_pose_denormalize_f32(const float* pose, int64_t n_frames, const float* mean,
                             const float* std_, float* out, void* stream);
int a2m_pck_f32(const float* pred, const float* gt, int32_t N, int32_t K, double alpha,
                double* out, void* stream);

/* PATS windowing (dataUtils.py:585-665): out[w][j][c] =
 * data[starts[w] + j*interval][c], j < ceil(window/interval), data [length][C] in HBM; with
 * mean/std (both or neither) each value is standardised as (x - mean[c]) / (std[c] < 1e-7 ? 1 : std[c]).
 * n_windows = 0 does nothing and accepts NULL data, starts and out. */
int a2m_window_gather_f32(const float* data, int64_t length, int32_t C, const int64_t* starts,
                          int32_t n_windows, int32_t window, int32_t interval, const float* mean,
                          const float* std_, float* out, void* stream);

/* One batch of the HBM-resident PATS loader (a2m.data.PatsLoader; dataUtils.py:638-665 and :745-758
 * for every clip of a DataLoader batch, and version5_model_train.py:296-319 for the poses) in one
 * launch.  For modality m < n_mod (1..A2M_BATCH_MAX_MOD), clip b < n and j < ceil(window[m] /
 * interval[m]):
 *   sample = order[b0 + b]
 *   out[m][b][j][:] = f(arena[m][start[m][sample] + j*interval[m]][:])
 * arena[m]: [rows][C[m]] float32, every interval of every split concatenated; start[m]: int64, the
 * arena row of each sample's window start; order: int64, the epoch's permutation.  order and
 * start are device arrays read by the kernel, so the launch has no host synchronisation, captures
 * into a HIP graph, and a replay after order was overwritten gathers the new clips.  The arrays
 * arena .. out are host arrays of n_mod entries, read during the call.
 * mode[m]: A2M_BATCH_RAW copies bitwise (mean[m] and std_[m] must be NULL); A2M_BATCH_STANDARDISE
 * is a2m_window_gather_f32's (x - mean[c]) / (std[c] < 1e-7 ? 1 : std[c]); A2M_BATCH_NECKSUB
 * (C[m] == 104 only) is a2m_pose_normalize_f32's ((x - neck) - mean[c]) / std[c], neck = column 0
 * for c < 52, else column 52.  Both need mean[m] and std_[m] ([C[m]] device floats).
 * C[m] % 4 == 0 and arena[m], out[m] 16-byte aligned: the kernel moves float4.  The kernel checks
 * no bounds: the caller guarantees order[b0 .. b0+n) valid samples and start + window within the
 * arena.  A2M_EINVAL before any launch for n_mod out of range, n < 0 or b0 < 0, and with n > 0 for a
 * NULL array, arena, start, out or order, window or interval <= 0, an unknown mode, or mean / std
 * not as the mode requires.  n = 0 returns A2M_OK without a launch and accepts NULL pointers. */
#define A2M_BATCH_MAX_MOD 4
#define A2M_BATCH_RAW 0
#define A2M_BATCH_STANDARDISE 1
#define A2M_BATCH_NECKSUB 2
int a2m_batch_gather_f32(int32_t n_mod, const float* const* arena, const int64_t* const* start,
                         const int32_t* C, const int32_t* window, const int32_t* interval,
                         const int32_t* mode, const float* const* mean, const float* const* std_,
                         float* const* out, const int64_t* order, int64_t b0, int32_t n, void* stream);

/* ---- Train-time augmentation inside the loader's gather (a2m.data.Augment; csrc/augment.hip) ----
 * a2m_augment_params_f32 fills params[b][8] (device float32) for the clips pos = order[b0 + b],
 * b < n, one launch, no host synchronisation.  Columns: mirror (0 / 1), s, g, gain, f0, fw, t0, tw.
 * The generator is Philox4x32-10 with key (seed & 0xffffffff, seed >> 32) and counter
 * (pos & 0xffffffff, pos >> 32, (uint32) pass[0], call); pass is a device int64[1] read by the kernel,
 * so a captured launch follows an overwritten pass number.  u = float(x >> 8) * 2^-24 of an output
 * word x.  Call 0, words 0..3: mirror = u0 < p_mirror; s = 1 + r_speed (2 u1 - 1);
 * g = 1 + r_scale (2 u2 - 1); gain = r_gain (2 u3 - 1).  Call 1: fw = floor(u0 (max_fw + 1));
 * f0 = floor(u1 (C - fw + 1)); tw = floor(u2 (max_tw + 1)); t0 = floor(u3 (T - tw + 1)).  Every
 * float step is rounded once to fp32 (2u and 2u - 1 are exact).  A clip's row depends on (seed,
 * pass[0], pos) only: not on n, b0 or b.
 * A2M_EINVAL ("augment_params: ...") before any launch: n < 0 or b0 < 0; p_mirror outside [0, 1];
 * r_speed outside [0, 0.5]; r_scale outside [0, 1); r_gain negative or not finite; C or T outside
 * 1 .. 2^24 - 1; max_fw outside [0, C]; max_tw outside [0, T]; with n > 0 a NULL order, pass or
 * params.  n = 0 returns A2M_OK without a launch.
 *
 * a2m_batch_gather_aug_f32 is a2m_batch_gather_f32 with the row b of params applied to clip b.
 * last[m]: int64 device table beside start[m], the arena row of the last row of each sample's
 * interval.  role[m]: A2M_AUGMENT_NONE, A2M_AUGMENT_POSE (mode A2M_BATCH_NECKSUB only) or
 * A2M_AUGMENT_AUDIO (modes RAW and STANDARDISE).  perm: int32[52] device table, the source joint of
 * each output joint of a mirrored clip (entries outside [0, 52) read the joint itself).
 *   tempo, every role: output frame j reads row position p = fl(float(j * interval[m]) * s) from the
 *     sample's start (clamped to [0, 2^24]); i = floor(p), f = p - i; a = row min(start + i, last),
 *     b = row min(start + i + 1, last); the value is a where f == 0 (row b is then not read, so
 *     s == 1 is a2m_batch_gather_f32 bit for bit) and a + f (b - a) otherwise, three roundings.
 *   A2M_BATCH_NECKSUB: d = v[src] - v[neck] over the interpolated channels of the same plane, src =
 *     perm[k] for a mirrored clip of the pose role, else k; pose role: d = -d in the x plane when
 *     mirrored, then d = d * g; out = (d - mean[c]) / std[c] with the output channel's statistics.
 *   audio role: gain, where non-zero, is added to the interpolated value before the mode's
 *     arithmetic; afterwards channels [f0, f0 + fw) of every frame and frames [t0, t0 + tw) of every
 *     channel are written as mask_fill.  A width of 0 masks nothing.
 * The kernel checks no bounds beyond the clamp at last: the caller guarantees order, start and last
 * as for a2m_batch_gather_f32, last >= start, and params [n][8].  No host synchronisation; captures
 * into a HIP graph.  A2M_EINVAL ("batch_gather_aug: ...") before any launch for everything
 * a2m_batch_gather_f32 refuses, a NULL last, role, params or perm, an unknown role, the pose role
 * on a mode other than NECKSUB, the audio role on NECKSUB, window >= 2^24.  n = 0 returns A2M_OK
 * without a launch and accepts NULL pointers. */
#define A2M_AUGMENT_NPARAM 8
#define A2M_AUGMENT_NONE 0
#define A2M_AUGMENT_POSE 1
#define A2M_AUGMENT_AUDIO 2
int a2m_augment_params_f32(const int64_t* order, int64_t b0, int32_t n, const int64_t* pass,
                           uint64_t seed, float p_mirror, float r_speed, float r_scale, float r_gain,
                           int32_t max_fw, int32_t C, int32_t max_tw, int32_t T, float* params,
                           void* stream);
int a2m_batch_gather_aug_f32(int32_t n_mod, const float* const* arena, const int64_t* const* start,
                             const int64_t* const* last, const int32_t* C, const int32_t* window,
                             const int32_t* interval, const int32_t* mode, const int32_t* role,
                             const float* const* mean, const float* const* std_, float* const* out,
                             const int64_t* order, int64_t b0, int32_t n, const float* params,
                             const int32_t* perm, float mask_fill, void* stream);

/* ---- Evaluation baselines over the loader's arena (a2m/baselines.py; csrc/baselines.hip) ----
 * Both entries address windows exactly as a2m_batch_gather_f32 does: the window at table position p
 * is the rows arena[start[p] + j*interval], j < T = ceil(window / interval), of an arena
 * [rows][C] float32, C % 4 == 0, arena 16-byte aligned.  They read the arena through the start
 * table in place: no [n][T*C] copy of the windows exists.  The kernels check no bounds: the caller
 * guarantees start[lo .. lo+n) and start + window within the arena.  No host synchronisation; the
 * launches (and one memset node of the median) capture into a HIP graph.
 *
 * a2m_nn_search_f32: for every query b < B (query [B][T][C], 16-byte aligned) and every table
 * position p in [lo, lo + n_cand)
 *   d(b,p) = sum_{j<T, c<C} (query[b][j][c] - f(arena[start[p] + j*interval][c]))^2
 * with f the identity for A2M_BATCH_RAW (mean, std_ NULL) and the gather's
 * (x - mean[c]) / (std[c] < 1e-7 ? 1 : std[c]) for A2M_BATCH_STANDARDISE (both given).  best[b]
 * (int64) is the absolute position p of the smallest computed d, the lowest p among bitwise-equal
 * values (so best serves as `order` with b0 = 0 of a2m_batch_gather_f32); best_dist[b] is that
 * value, clamped at 0.  d is computed as (|q|^2 + |w|^2) - 2 q.w in fp32: q.w on the exact fp32
 * MFMA as one k-ordered fma chain per (b, p), the two norms as fixed fma chains and a fixed
 * 16-lane tree.  The computed d(b,p) is a function of the query's and the window's values alone
 * (not of p's place in the table, a tile or a chunk), and the result does not depend on workgroup
 * scheduling: every candidate chunk writes its own (distance bits, p) minimum per query into ws,
 * and a second small launch takes the minimum over the chunks.  Error: |d - exact| <=
 * 4 K 2^-24 (|q|^2 + |w|^2), K = T*C.  Inputs must be finite.  ws: a2m_nn_search_ws_bytes(B, n_cand)
 * bytes, 8-byte aligned.
 * A2M_EINVAL before any launch: a NULL arena, start, query, best, best_dist or ws; B, n_cand,
 * window or interval <= 0; C <= 0 or C % 4; lo < 0; a mode other than RAW / STANDARDISE; mean /
 * std_ not as the mode requires; arena, query, mean or std_ not 16-byte aligned; ws_bytes too small; n_cand > 2^31 - 2^16
 * or T*C > 2^30 (32-bit candidate and k indices). */
size_t a2m_nn_search_ws_bytes(int32_t B, int64_t n_cand);
int a2m_nn_search_f32(const float* arena, const int64_t* start, int64_t lo, int64_t n_cand, int32_t C,
                      int32_t window, int32_t interval, int32_t mode, const float* mean,
                      const float* std_, const float* query, int32_t B, int64_t* best,
                      float* best_dist, void* ws, size_t ws_bytes, void* stream);

/* a2m_window_median_f32: out[c], c < C, is the exact median (numpy.median's value) of the multiset
 * { g(row)[c] : row of window p, p in [lo, lo + n) }, M = n*T values; a frame shared by overlapping
 * windows counts once per window.  g is the identity for A2M_BATCH_RAW and, for A2M_BATCH_NECKSUB
 * (C == 104), x[c] - x[neck] (one fp32 subtraction), neck = column 0 for c < 52, else column 52.
 * M odd: the middle element; M even: the two middle elements added in double, halved and rounded
 * once to float.  Inputs must be finite.  A radix select on the order-preserving integer image of
 * the float, 8 bits a pass, four passes, both ranks carried at once; the bucket of each pass is
 * chosen on the device.  ws: a2m_window_median_ws_bytes(C) bytes, 4-byte aligned.
 * A2M_EINVAL before any launch: a NULL arena, start, out or ws; n, window or interval <= 0; C <= 0,
 * C % 4 or C > 2^20; lo < 0; a mode other than RAW / NECKSUB; NECKSUB with C != 104; a misaligned
 * arena; ws_bytes too small; n*T >= 2^32 (32-bit ranks and counts). */
size_t a2m_window_median_ws_bytes(int32_t C);
int a2m_window_median_f32(const float* arena, const int64_t* start, int64_t lo, int64_t n, int32_t C,
                          int32_t window, int32_t interval, int32_t mode, float* out, void* ws,
                          size_t ws_bytes, void* stream);

/* ---- Sample-level set metrics of the test epoch (a2m.evaluation.CoverageEvaluator; csrc/coverage.hip) ----
 * Precision / recall, density / coverage and diversity over whole clips from four
 * kernels.  All take a stream, issue no host synchronisation, use no atomics and no workspace
 * shared between workgroups, and give byte-identical results from run to run.  Inputs must be finite.
 *
 * a2m_coverage_store_f32: the feature rows of one batch.  fake_norm, real_px [n][T][Fd] float32,
 * style int32[n], mean / std_ [Fd]; rows row0 .. row0 + n of feat_fake and feat_real [capacity][D]
 * and of styles int32[capacity] are written.  A2M_COVERAGE_POSE (D = T*Fd): the generated clip as it
 * is, the real clip (x - mean[c]) / (std[c] < 1e-7 ? 1 : std[c]), one rounding a step (the loader's
 * gather formula).  A2M_COVERAGE_MOTION (D = (T-1)*Fd): x[t+1] - x[t] of those, one fp32
 * subtraction each.  row0 is a host value: successive batches are not one replayable graph node.
 * A2M_EINVAL ("coverage_store: ...") before any launch: a NULL pointer; an unknown feature; n <= 0;
 * T < 1 (motion: T < 2); Fd <= 0 or Fd % 4; row0 < 0 or row0 + n > capacity; poses, statistics or
 * feature buffers not 16-byte aligned; D > 2^30 or n*D >= 2^40.
 *
 * a2m_pair_dist2_f32: slab[i][j] (row-major [nA][nB] float32) =
 *   max((|a_i|^2 + |b_j|^2) - 2 a_i.b_j, 0),  a_i = feat_a[rows_a[i]], b_j = feat_b[rows_b[j]]
 * for device int32 row lists into feature buffers [cap][D]; a row number outside [0, cap) is read
 * as the nearest valid row, so no list makes the kernel read outside the buffers.  a.b on the
 * exact fp32 MFMA (v_mfma_f32_32x32x2_f32) as one k-ordered fma chain per element, the norms as
 * fixed fma chains and a fixed 16-lane tree: the value is a function of the two vectors alone, and
 * equal vectors give bitwise-equal distances wherever they sit.  Error: |d2 - exact| <=
 * 4 D 2^-24 (|a|^2 + |b|^2); two identical vectors get a distance within that of 0, not
 * necessarily 0.  exclude_self = 1 writes +inf at (i, diag0 + i): rows_a is then the sub-list of
 * rows_b that starts at its position diag0.  The slab is the workspace: slab_bytes >=
 * a2m_pair_dist2_ws_bytes(nA, nB) = 4 nA nB (0 for sizes the entry refuses).
 * A2M_EINVAL ("pair_dist2: ...") before any launch: a NULL pointer; nA, nB, a capacity <= 0; D <= 0
 * or D % 4; D > 2^30; nA > 65535 * 64; nB > 2^31 - 2^16; a capacity > 2^31 - 1; exclude_self not
 * 0 / 1; diag0 < 0, diag0 != 0 without exclude_self, diag0 + nA > nB with it; misaligned feature
 * buffers (16 bytes), row lists or slab (4); slab_bytes too small.
 *
 * a2m_row_kth_f32: per row of a slab [nA][nB] whose values are >= +0 or +inf, kth[row] = the k-th
 * smallest value (1 <= k <= 32), exact, ties ordered by column (selection on the 64-bit key
 * bits << 32 | column), and sums[row] (float64) = the sum of sqrt((double) v) over the row's finite
 * entries: every lane of the row's wave adds its columns lane, lane + 64, ... in ascending order,
 * then a butterfly over the lanes.  exclude_self = 1 says that every row holds one +inf of its own.
 * A2M_EINVAL ("row_kth: ...") before any launch: a NULL pointer; nA or nB <= 0 or > 2^31 - 2^16;
 * k outside 1..32; exclude_self not 0 / 1; k > nB - exclude_self; misaligned pointers.
 *
 * a2m_row_cover_f32: per row of such a slab, count[row] (int32) = #{j : slab[row][j] <= r2[j]} and
 * rowmin[row] = the row's smallest value.
 * A2M_EINVAL ("row_cover: ...") before any launch: a NULL pointer; nA or nB <= 0 or > 2^31 - 2^16;
 * misaligned pointers. */
#define A2M_COVERAGE_POSE 0
#define A2M_COVERAGE_MOTION 1
int a2m_coverage_store_f32(const float* fake_norm, const float* real_px, const int32_t* style,
                           const float* mean, const float* std_, int32_t n, int32_t T, int32_t Fd,
                           int32_t feature, int64_t row0, int64_t capacity, float* feat_fake,
                           float* feat_real, int32_t* styles, void* stream);
size_t a2m_pair_dist2_ws_bytes(int64_t nA, int64_t nB);
int a2m_pair_dist2_f32(const float* feat_a, int64_t cap_a, const int32_t* rows_a, int64_t nA,
                       const float* feat_b, int64_t cap_b, const int32_t* rows_b, int64_t nB, int64_t D,
                       int32_t exclude_self, int64_t diag0, float* slab, size_t slab_bytes, void* stream);
int a2m_row_kth_f32(const float* slab, int64_t nA, int64_t nB, int32_t k, int32_t exclude_self, float* kth,
                    double* sums, void* stream);
int a2m_row_cover_f32(const float* slab, int64_t nA, int64_t nB, const float* r2, int32_t* count,
                      float* rowmin, void* stream);

/* ---- Train samplers over the loader's arena (a2m/sampling.py; csrc/sampling.hip) ----
 * The device half of PatsLoader.train_sampler: the mean joint speed of every clip of a split, exact
 * order statistics of those speeds, and the binning of the clips.  All three take a stream, issue no
 * host synchronisation, capture into a HIP graph (one memset node ahead of the velocity and the
 * classify kernel, one ahead of the select passes), use no floating-point atomics, and give
 * byte-identical results from run to run.
 *
 * a2m_clip_velocity_f32: clip i in [lo, lo + n) of a start table is the rows r_t = start[i] +
 * t*interval, t < T = ceil(window / interval), of arena [rows][C] float32 in the loader's planar
 * pose layout: K = C/2 joints, x of joint j in channel j, y in channel K + j, joint 0 the neck.
 *   out[i - lo] = mean over t = 1 .. T-1 and j = 1 .. K-1 of
 *                 sqrt((x[r_t][j] - x[r_t-1][j])^2 + (x[r_t][K+j] - x[r_t-1][K+j])^2)
 * the mean 2-D speed of the non-neck joints in pixels per frame.  Every term is computed in fp32
 * (two differences, the sum of squares, a correctly rounded root); one wave owns a clip, every lane
 * adds its terms in double in a fixed order, the lanes are combined by a fixed tree, and the mean
 * is rounded once to float: the value is a function of the clip's rows alone.  n_nonfinite (device
 * int32, zeroed here) receives the number of clips whose result is not finite (an integer atomic).
 * The kernel checks no bounds: the caller guarantees start[lo .. lo+n) and start + window within
 * the arena.
 * A2M_EINVAL ("clip_velocity: ...") before any launch: n < 0 or lo < 0; with n > 0 a NULL arena,
 * start, out or n_nonfinite; C odd or C < 4 (fewer than two joints); window <= 0 or interval <= 0;
 * T < 2; (T-1)*(K-1) or n >= 2^31.  n == 0 is A2M_OK without a launch, whatever the other arguments.
 *
 * a2m_select_f32: out[w] = the element at rank ranks[w] (host int64[k], 1 <= k <=
 * A2M_SELECT_MAX_RANKS, 0 <= rank < n, repeats allowed) of the ascending order of the n values x
 * (device float32, every one non-negative and finite: such floats order as their bit patterns, which
 * is what is compared, so +0 and subnormals keep their place); minmax[0], minmax[1] the smallest and
 * the largest.  A radix select, 8 bits a pass from the top, four passes, every rank carried at once:
 * a histogram kernel (LDS and global integer atomics) and a one-wave kernel that walks the 256
 * counts to each rank's bucket; the bucket is chosen on the device.  Exact.  ws:
 * a2m_select_f32_ws_bytes(n) bytes, 4-byte aligned.
 * A2M_EINVAL ("select: ...") before any launch: n < 0 or n >= 2^32; with n > 0 a NULL x, ranks, out,
 * minmax or ws; k outside 1..A2M_SELECT_MAX_RANKS; a rank outside [0, n); ws misaligned or ws_bytes
 * too small.  n == 0 is A2M_OK without a launch.
 *
 * a2m_classify_f32: cls[i] (device int32) is the class of x[i] (device float32) against thr (host
 * double[n_thr]; the comparison is done in double, to which the float converts exactly), counts[c]
 * (device int64[n_cls], zeroed here) the number of elements of class c, n_cls = 1 for ABOVE and
 * TAIL and n_thr - 1 for BINS; integer adds only.
 *   A2M_CLASSIFY_ABOVE (n_thr 1)  0 if x > thr[0], else -1
 *   A2M_CLASSIFY_TAIL  (n_thr 2)  0 if x > thr[1] or x < thr[0], else -1
 *   A2M_CLASSIFY_BINS  (n_thr q+1 ascending edges)  the first j with thr[j] <= x <= thr[j+1]: both
 *                      ends closed, a value on an inner edge in the lower bin; -1 if none (NaN too)
 * A2M_EINVAL ("classify: ...") before any launch: n < 0; an unknown kind; with n > 0 a NULL x, thr,
 * cls or counts; n_thr not as the kind requires (BINS: 2 .. A2M_CLASSIFY_MAX_THR); a NaN threshold;
 * BINS edges that descend.  n == 0 is A2M_OK without a launch. */
#define A2M_SELECT_MAX_RANKS 8
#define A2M_CLASSIFY_ABOVE 0
#define A2M_CLASSIFY_TAIL 1
#define A2M_CLASSIFY_BINS 2
#define A2M_CLASSIFY_MAX_THR 257
int a2m_clip_velocity_f32(const float* arena, const int64_t* start, int64_t lo, int64_t n, int32_t C,
                          int32_t window, int32_t interval, float* out, int32_t* n_nonfinite,
                          void* stream);
size_t a2m_select_f32_ws_bytes(int64_t n);
int a2m_select_f32(const float* x, int64_t n, const int64_t* ranks, int32_t k, float* out,
                   float* minmax, void* ws, size_t ws_bytes, void* stream);
int a2m_classify_f32(const float* x, int64_t n, int32_t kind, const double* thr, int32_t n_thr,
                     int32_t* cls, int64_t* counts, void* stream);

/* ---- Pose video and track stitching ----
 * a2m_render_poses_u8 stands in for the drawing of generate_motion_video.py:66-164
 * (plot_head/body/hand_keypoints, draw_pose, draw_side_by_side_poses): every frame's P poses, each
 * a set of L polylines over its K keypoints, drawn into planar uint8 frames out[N][3][H][W].
 * kp [N][P][2][K] (x row, y row), xform [P][4] = sx, tx, sy, ty (px = sx*x + tx, py = sy*y + ty)
 * and out are DEVICE pointers.  poly_idx (the keypoint indices of all polylines, concatenated),
 * poly_off [L+1] (offsets into poly_idx, poly_off[0] = 0), poly_rgb [L][3] and bg [3] are HOST
 * pointers: the tables are validated here (every polyline >= 2 indices, 0 <= index < K) and travel
 * to the kernel by value, so the call allocates nothing, needs no workspace, is stream-ordered and
 * can be captured in a HIP graph.  Limits: L <= A2M_RENDER_MAX_POLYLINES, poly_off[L] <=
 * A2M_RENDER_MAX_INDICES, P*K <= A2M_RENDER_MAX_POINTS (the frame's keypoints are staged in LDS),
 * P * ceil(poly_off[L] / 64) <= A2M_RENDER_MAX_CHUNKS (one culling mask per 64 segments of a pose).
 * Pixel function: the centre of pixel (i, j) is (i + 0.5, j + 0.5); for one polyline of one pose d
 * is the smallest distance from the centre to any of its segments (zero length: a point; a segment
 * with a non-finite endpoint is skipped), its coverage c = clamp(half_width_px + 0.5 - d, 0, 1);
 * per channel v = bg, then for p = 0..P-1, l = 0..L-1: v = v*(1 - c) + rgb[l]*c; the byte stored
 * is (uint8)(v + 0.5f).  Blending is affine, so a palette and background converted to YCbCr give
 * the Y, Cb and Cr planes of the same picture.  matplotlib's Agg output (butt caps, its own
 * anti-aliasing) is NOT reproduced: the float64 restatement in tests/render_ref.py is the pin.
 * A2M_EINVAL: a null pointer with N > 0; P, K, W or H < 1, L < 0; a polyline shorter than 2
 * indices; an index outside [0, K); half_width_px negative or not finite; a limit exceeded.
 * N = 0 returns A2M_OK without a launch and accepts NULL pointers. */
#define A2M_RENDER_MAX_POLYLINES 128
#define A2M_RENDER_MAX_INDICES 512
#define A2M_RENDER_MAX_POINTS 4096
#define A2M_RENDER_MAX_CHUNKS 1024
int a2m_render_poses_u8(const float* kp, int32_t N, int32_t P, int32_t K, const int32_t* poly_idx,
                        const int32_t* poly_off, const uint8_t* poly_rgb, int32_t L,
                        const float* xform, float half_width_px, const uint8_t bg[3], int32_t W,
                        int32_t H, uint8_t* out, void* stream);

/* a2m_track_blend_f32 stitches the windows that generate_motion_video.py:247-260 produces one
 * batch at a time into one track, de-normalising (:259-260) in the same pass.  win [n][T][Fd] are
 * windows whose starts lie h = T - overlap frames apart (0 <= overlap <= T/2); out
 * [(n-1)*h + T][Fd].  Gather form: an output frame reads one window, or two inside an overlap,
 * where frame j of window k weighs (j + 0.5)/overlap at its head (k > 0, j < overlap) and
 * (T - j - 0.5)/overlap at its tail (k < n-1, j >= T - overlap): the two weights sum to 1.
 * out = sum w*win, then *std + mean when given (both or neither, [Fd]).  A frame of a single
 * window is copied bit for bit, or equals a2m_pose_denormalize_f32 bit for bit; overlap = 0 is a
 * concatenation.  No atomics: deterministic.  A2M_EINVAL: T or Fd < 1, n < 0, overlap out of
 * range, one of mean / std alone, null win or out with n > 0.  n = 0 returns A2M_OK. */
int a2m_track_blend_f32(const float* win, int32_t n, int32_t T, int32_t Fd, int32_t overlap,
                        const float* mean, const float* std_, float* out, void* stream);
/* The same track, m >= 0 new consecutive windows win [m][T][Fd] at a time.  tail [overlap][Fd] is
 * device state owned by the caller: frames [h, T) of the last window seen, normalised; has_prev
 * says whether it holds one (0 at the start of a stream).  The call writes the m*h frames that the
 * new windows make final to out (the first `overlap` of them cross-faded with the tail when
 * has_prev), then rewrites the tail from window m - 1.  flush != 0 also writes, after them, the
 * `overlap` tail frames of the last window unblended: the end of the stream; out is then
 * [m*h + overlap][Fd].  Every element goes through a2m_track_blend_f32's own arithmetic, so the
 * calls of a stream, concatenated, equal the offline track bit for bit.  No atomics; each tail
 * element is read and rewritten by one thread.  A2M_EINVAL: T or Fd < 1, m < 0, overlap out of
 * range, one of mean / std alone, a flush with m = 0 and no window before it, a null win, tail
 * (overlap > 0) or out where it is needed.  m = 0 without flush returns A2M_OK.  No allocation, no
 * host synchronisation: capturable. */
int a2m_track_blend_stream_f32(const float* win, int32_t m, int32_t T, int32_t Fd, int32_t overlap,
                               float* tail, int32_t has_prev, int32_t flush, const float* mean,
                               const float* std_, float* out, void* stream);

/* ---- Baseline JPEG of rendered frames (generate_motion_video.py:174-185 writes %04d.jpg) ----
 * a2m_jpeg_encode_u8 turns frames [N][3][H][W] (uint8 planes that already hold Y, Cb, Cr in full
 * range, JFIF BT.601, as a2m_render_poses_u8 writes them from a converted palette) into the
 * entropy-coded scans of baseline sequential JPEG files: SOF0, 8-bit, three components, 4:4:4
 * (every sampling factor 1), one interleaved scan.  The scans are compacted back to back in `out`;
 * offsets [N+1] (int64, DEVICE) receives each frame's first byte and, in offsets[N], the total.
 * The header (SOI .. SOS) and EOI are the caller's (a2m/jpeg.py: jpeg_header); the scan depends on
 * nothing in them but the tables below.  frames, out, offsets and ws are DEVICE pointers; qluma and
 * qchroma are HOST pointers to 64 quantisers each in natural order (entry 8v + u divides
 * coefficient (v, u)) and travel to the kernels by value.
 *
 * The byte stream (tests/jpeg_ref.py restates it; the device bytes equal it bit for bit).
 *  Blocks.  MW = ceil(W/8), MH = ceil(H/8) MCUs of one 8x8 block per component, in the order
 *   Y, Cb, Cr.  Pixel (8r + y, 8m + x) of block (r, m) is read at (min(., H-1), min(., W-1)): the
 *   last row and column are replicated into the edge blocks.
 *  Level shift and DCT, in 32-bit integers.  s[y][x] = pixel - 128.  M[u][x] =
 *   round(2^13 * c(u)/2 * cos((2x+1) u pi/16)) with c(0) = 1/sqrt(2), c(u>0) = 1: M[0][x] =
 *   A2M_JPEG_C0 and, for u > 0, M[u][x] = +-A2M_JPEG_Ck with k pi/16 the angle folded into the
 *   first quadrant.  Rows first, t[y][u] = (sum_x s[y][x] M[u][x] + 2^6) >> 7 (six fraction bits
 *   kept), then columns, d[v][u] = (sum_y t[y][u] M[v][y] + 2^18) >> 19.  >> is arithmetic: both
 *   roundings are floor(z + 1/2).  Largest |sum|: 2.97e6, then 5.4e8.
 *  Quantisation.  q = sign(d) * ((2 |d| + Q) / (2 Q)), the division truncating: |d| / Q rounded
 *   half away from zero.  |q| is then limited to 1024 (DC) or 1023 (AC), which no input reaches
 *   (|d| <= 1024 and <= 928) and which guarantees a code for every symbol.
 *  Entropy coding.  Zig-zag order; DC as the difference to the previous block of the same
 *   component; Huffman tables: the typical tables K.3-K.6 of ITU-T T.81 Annex K (luma tables for
 *   Y, chroma tables for Cb and Cr), which code all 12 DC categories and all 162 AC symbols; value
 *   bits as T.81 F.1.2; ZRL for runs of 16 zeros; EOB unless coefficient 63 is nonzero.
 *  Restart intervals.  One MCU row is one interval (DRI = MW): the DC predictors start at 0 in
 *   each, its last byte is filled with 1-bits, every 0xFF byte is followed by 0x00, and every
 *   interval but a frame's last is followed by RSTn, n = r mod 8 for MCU row r.  A frame's scan
 *   ends with its last interval's last byte (EOI is not written).
 *
 * Capacity.  `capacity` is the size of `out` in bytes.  offsets is always written in full; bytes
 * at or past the capacity are dropped, never written.  offsets[N] > capacity therefore is the
 * overflow flag and offsets[N] the size a second call needs (out may be NULL with capacity 0, to
 * size alone).  ws: a2m_jpeg_ws_bytes(N, W, H) bytes (the quantised coefficients, the blocks' bit
 * positions, A2M_JPEG_MAX_BLOCK_BYTES of scan scratch per block: 22 bits of DC and 63 x 26 bits of
 * AC at most); the call allocates nothing, is six stream-ordered launches and can be captured in
 * a HIP graph.  The only atomics OR disjoint bits into zeroed words, so the bytes are a pure
 * function of the input.  A2M_EINVAL: a null pointer with N > 0; N < 0; W or H < 1 or > 65535; a
 * quantiser of 0 or above 255 (baseline tables are 8-bit); capacity < 0; ws_bytes too small; more
 * than INT32_MAX intervals (N ceil(H/8)) or 4 INT32_MAX blocks (one launch covers them).
 * N = 0 returns A2M_OK without a launch and accepts NULL pointers. */
#define A2M_JPEG_C0 2896 /* 2^12 / sqrt(2) */
#define A2M_JPEG_C1 4017 /* 2^12 cos(1 pi/16) */
#define A2M_JPEG_C2 3784
#define A2M_JPEG_C3 3406
#define A2M_JPEG_C4 2896
#define A2M_JPEG_C5 2276
#define A2M_JPEG_C6 1567
#define A2M_JPEG_C7 799
#define A2M_JPEG_PASS1_SHIFT 7
#define A2M_JPEG_PASS2_SHIFT 19
#define A2M_JPEG_MAX_BLOCK_BYTES 208
size_t a2m_jpeg_ws_bytes(int32_t N, int32_t W, int32_t H); /* 0 for sizes the encoder refuses */
int a2m_jpeg_encode_u8(const uint8_t* frames, int32_t N, int32_t W, int32_t H,
                       const uint16_t* qluma, const uint16_t* qchroma, uint8_t* out,
                       int64_t capacity, int64_t* offsets, void* ws, size_t ws_bytes, void* stream);

/* Measurement hook (bench.py): while enabled, every launch of the implicit-GEMM engine (up to
 * 1024 per window; more make _read fail) carries a record of span stamps that its tile kernel and
 * split-K reduce write themselves (earliest block start, latest wave end on the GPU's constant-rate
 * wall clock, which all XCDs share; a span is last end - first start over all XCDs), eagerly or inside a graph
 * captured while enabled.  _read synchronises the device and returns the launch count, the
 * launches' algorithmic FLOPs (2*M*N*K*batch), the summed tile-kernel spans and the summed
 * split-K reduce spans (ms) of the latest execution, then re-arms the stamps (so it can follow
 * each replay of such a graph); _stop ends recording of new launches, _end = _stop + _read +
 * forget the records.  No effect when disabled. */
int a2m_gemm_timing_begin(void);
/* Tuning hook: force the engine's tile (64 | 128) and split-K count for subsequent launches
 * (0 = the planner's choice); workspace sizing follows.  Process-global, not for production. */
int a2m_gemm_plan_override(int32_t tile, int32_t splits);
/* Test / tuning hook: which 64x64 tile kernel eligible launches take -- 1 the software-pipelined
 * tile (gemm_pipe.h / gemm_pipe_bf16.h), 0 gemm_tile, -1 the default
 * (1).  Both give bitwise-equal results; process-global, not for production. */
int a2m_gemm_pipe_override(int32_t mode);
/* Test / tuning hook: whether a2m_convt1d_tap_fwd_f32 issues the two output phases of a stride-2
 * layer as one paired launch of the fp32 pipelined tile (each phase at one split) -- 1 wherever
 * the engine can take both phases, 0 never (one launch per phase, as every other geometry), -1 the
 * default: as 1, but only where the pair puts at least one 64x64 tile on every CU.  Each phase's
 * result is bitwise that of its own launch at one split; process-global, not for production. */
int a2m_convt_pair_override(int32_t mode);
/* Test hook: V channels per workgroup of the fused eval SelfAttention at C % 128 == 0 -- 64
 * (default: eight waves, Q / K computed by each of the C / 64 chunks) or 128 (twelve waves, Q / K
 * once per two 64-channel chunks: less kernel time, but measured 0.5-0.7 % slower a step).  Both
 * give bitwise-equal results; A2M_EINVAL for any other value.  Process-global, not for
 * production. */
int a2m_set_attn_eval_chunk(int32_t nv);
/* Operand precision of every GEMM-engine launch (convs, linears, attention products and their
 * backward) issued after the call: 0 = fp32 (default; the parity configuration), 1 = bf16
 * operands with fp32 accumulation (BASELINE configs[4], torch.autocast(bfloat16)-equivalent:
 * weights and activations stay fp32 in HBM, rounded to bf16 where they enter the MFMA),
 * (2 = bf16x6, fp32 operands split into three bf16 pieces, six products: only in a library built
 * with -DA2M_WITH_X6, an experiment measured slower than fp32; A2M_EINVAL otherwise).
 * Process-wide; not thread-safe against concurrent launches. */
int a2m_set_gemm_precision(int32_t prec);
int32_t a2m_get_gemm_precision(void);
int a2m_gemm_timing_end(int64_t* launches, double* flops, double* ms_tile, double* ms_reduce,
                        int64_t* reduces);
int a2m_gemm_timing_stop(void);
/* Per-launch tile-kernel spans of the latest execution instead of their sums: the first block
 * start and last block end (us on the GPU wall clock, -1 for a launch that did not run) of the
 * first min(cap, launches) records; re-arms the stamps like _read. */
int a2m_gemm_timing_read_spans(int64_t cap, double* start_us, double* end_us, int64_t* n);
/* _read_spans plus each launch's ready mark (us; -1 unless A2M_GEMM_TIMING_READY=1 was set when
 * the launch was recorded: the wall clock at which a one-thread mark kernel enqueued right before
 * the tile kernel ran, i.e. when its stream reached the launch) */
int a2m_gemm_timing_read_spans_ex(int64_t cap, double* ready_us, double* start_us, double* end_us,
                                  int64_t* n);
/* _stop + forget the records without reading them (after the last _read of a kept window) */
int a2m_gemm_timing_clear(void);
int a2m_gemm_timing_read(int64_t* launches, double* flops, double* ms_tile, double* ms_reduce,
                         int64_t* reduces);
/* _read plus ms_queued: the sum over launches of (last block end - ready mark), the launch's time
 * from the moment its stream reached it, i.e. including its dispatch and any wait for free CUs
 * (0 without A2M_GEMM_TIMING_READY=1) */
int a2m_gemm_timing_read_ex(int64_t* launches, double* flops, double* ms_tile, double* ms_reduce,
                            int64_t* reduces, double* ms_queued);
/* Named wall-clock marks (measurement only; after a2m_gemm_timing_begin has allocated the stamp
 * buffer): a one-thread kernel on the stream stores the GPU wall clock into mark `slot`
 * (0 .. A2M_TIMING_MARKS-1), also as a node of a graph being captured; _elapsed synchronises the
 * device and returns mark b - mark a in ms. */
#define A2M_TIMING_MARKS 16
int a2m_timing_mark(int32_t slot, void* stream);
int a2m_timing_mark_elapsed(int32_t a, int32_t b, float* ms);
/* ms from mark `slot` to the last block end (tile kernel or its split-K reduce) of engine
 * launch record `rec` of the current timing window, in the latest execution (does not re-arm) */
int a2m_timing_mark_to_launch_end(int32_t slot, int64_t rec, float* ms);

#ifdef __cplusplus
}
#endif
#endif /* A2M_H_ */
