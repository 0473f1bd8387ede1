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

}  // namespace dcx
