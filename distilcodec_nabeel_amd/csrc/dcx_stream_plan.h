// Token streams (dcx_stream_decode_step, DESIGN.md §3 "Token streams"): one step of a session slot's
// counters.  The one definition of the arithmetic: the plan kernel (dcx_stream.hip) runs it per slot on
// the device, dcx_stream_plan_step runs it on the host, where callers mirror the counters instead of
// reading them back.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DCX_STREAM_HD __host__ __device__
#else
#define DCX_STREAM_HD
#endif

namespace dcx {

enum { STREAM_FINAL = 1, STREAM_RESTART = 2 };

// A slot: T codes received, E frames whose audio was emitted, closed after FINAL.
// One step's outputs: the window is codes [T - len, T) (len <= push + 2 halo), of which rows
// [skip, skip + take) are emitted; t_old is T before the step's n codes were appended (n: the caller's
// count clamped to [0, push], 0 for a closed slot).
struct StreamSlot {
  int T, E, closed;
};
struct StreamStep {
  int len, skip, take, t_old, n;
};

DCX_STREAM_HD inline StreamStep stream_plan_step(int halo, int push, StreamSlot& s, int n, int flags) {
  // counters no step can have left behind (a state buffer that was never reset) start the slot over
  if (s.T < 0 || s.E < 0 || s.E > s.T || s.T - s.E > halo) flags |= STREAM_RESTART;
  if (flags & STREAM_RESTART) s.T = s.E = s.closed = 0;
  n = n < 0 ? 0 : n > push ? push : n;
  if (s.closed) n = 0;
  if (n > 0x7fffffff - s.T) n = 0x7fffffff - s.T;  // the frame counter saturates (2^31 frames: 266 days of audio)
  StreamStep o;
  o.t_old = s.T;
  o.n = n;
  s.T += n;
  const bool fin = (flags & STREAM_FINAL) != 0;
  const int g0 = s.E > halo ? s.E - halo : 0;
  const int f_new = fin ? s.T : (s.T - halo > s.E ? s.T - halo : s.E);
  o.len = s.T - g0;
  o.skip = s.E - g0;
  o.take = f_new - s.E;
  s.E = f_new;
  if (fin) s.closed = 1;
  return o;
}

// Audio streams (dcx_stream_encode_step, DESIGN.md §3 "Audio streams"): the same for the encoder side.
// A slot: M raw samples received, C codes emitted, closed after FINAL.  The STFT framing decides the
// counts: a clip of m raw samples has audio_frames(m) frames (dcx_num_frames(m + 1): the reference's
// leading zero; none while the reflect pad does not fit), of which the first audio_avail(m) touch no
// sample reflected at the clip's end; the first audio_margin() frames of a window read its left
// reflect pad and the leading zero.
struct AudioGeom {
  int hop, n_fft, pad, padr;
};
DCX_STREAM_HD inline int audio_frames(const AudioGeom& g, int m) {
  const long long len = (long long)m + 1 + g.pad + g.padr;
  return m < g.pad || len < g.n_fft ? 0 : (int)((len - g.n_fft) / g.hop + 1);
}
DCX_STREAM_HD inline int audio_need(const AudioGeom& g) { return g.n_fft - g.pad - 1; }  // 639: frame 0's last raw sample + 1
DCX_STREAM_HD inline int audio_avail(const AudioGeom& g, int m) {
  return m >= audio_need(g) ? (m - audio_need(g)) / g.hop + 1 : 0;
}
DCX_STREAM_HD inline int audio_margin(const AudioGeom& g) { return (g.pad + g.hop - 1) / g.hop; }
// The bounds of a geometry (push: raw samples per step, halo: frames): the longest window in samples
// (a multiple of hop), and the most frames one step emits (at FINAL).
DCX_STREAM_HD inline long long audio_window_samples(const AudioGeom& g, int halo, int push) {
  const long long w = (long long)push + (long long)g.hop * (2LL * halo + audio_margin(g)) + audio_need(g) - 1;
  return (w + g.hop - 1) / g.hop * g.hop;
}
DCX_STREAM_HD inline long long audio_take_max(const AudioGeom& g, int halo, int push) {
  return halo + ((long long)push + audio_need(g)) / g.hop;
}

struct AudioSlot {
  int M, C, closed;
};
// One step's outputs: the window is raw samples [start, M) (start a multiple of hop), len of them, 0 when
// the step emits nothing (the slot is then dead in the step's tokenization); window frames
// [skip, skip + take) are emitted; m_old is M before the step's n samples were appended.
struct AudioStep {
  int len, start, skip, take, m_old, n;
};

DCX_STREAM_HD inline AudioStep audio_plan_step(const AudioGeom& g, int halo, int push, AudioSlot& s, int n, int flags) {
  // counters no step can have left behind (a state buffer that was never reset) start the slot over
  if (s.M < 0 || s.C < 0 || (s.closed != 0 && s.closed != 1) || s.C > audio_frames(g, s.M) ||
      (long long)s.M - (long long)s.C * g.hop > (long long)halo * g.hop + audio_need(g) - 1)
    flags |= STREAM_RESTART;
  if (flags & STREAM_RESTART) s.M = s.C = s.closed = 0;
  n = n < 0 ? 0 : n > push ? push : n;
  if (s.closed) n = 0;
  if (n > 0x7ffffffe - s.M) n = 0x7ffffffe - s.M;  // the sample counter saturates (2^31 samples: a day of audio)
  AudioStep o;
  o.m_old = s.M;
  o.n = n;
  s.M += n;
  const bool fin = (flags & STREAM_FINAL) != 0;
  const int a = s.C - halo - audio_margin(g) > 0 ? s.C - halo - audio_margin(g) : 0;
  int c_new = fin ? audio_frames(g, s.M) : audio_avail(g, s.M) - halo;
  if (c_new < s.C) c_new = s.C;
  o.start = a * g.hop;
  o.skip = s.C - a;
  o.take = c_new - s.C;
  o.len = o.take > 0 ? s.M - o.start : 0;
  s.C = c_new;
  if (fin) s.closed = 1;
  return o;
}

}  // namespace dcx
