// Token streams on gfx950 (dcx_stream_decode_step; DESIGN.md §3 "Token streams"): the three kernels
// around the ragged decode of one step, for every session slot in one launch each.
//  * stream_plan: one thread per slot runs stream_plan_step (dcx_stream_plan.h) on the slot's counters
//    and leaves the step's window length, the rows to emit and the counters after the step;
//  * stream_window: the slot's window of codes, frames [T - len, T), from the code ring and the codes
//    this step appends, which it stores into the ring.  The ring holds frame f at row f % W and a
//    window is at most W frames, so the rows read (frames below the old T) and the rows written
//    (frames from it on) are distinct rows: no thread reads what another writes;
//  * stream_emit: the emitted frames of the window's waveform as 16-byte copies, zeros behind them,
//    and the commit of the counters.  A step whose decode was refused launches no emit kernel, so it
//    leaves every slot as it was.
// All are streaming kernels of a few KB per slot; blockIdx.y is the slot.
#include "dcx_kernels.h"
#include "dcx_stream_plan.h"

#include <algorithm>

namespace dcx {

typedef float f32x4s __attribute__((ext_vector_type(4)));

__global__ void __launch_bounds__(256) stream_plan_kernel(const StreamState st, const int* __restrict__ n_new,
                                                           const int* __restrict__ flags) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= st.sessions) return;
  StreamSlot s{st.T[b], st.E[b], st.closed[b]};
  const StreamStep o = stream_plan_step(st.halo, st.push, s, n_new[b], flags[b]);
  st.T_next[b] = s.T;
  st.E_next[b] = s.E;
  st.closed_next[b] = s.closed;
  st.len[b] = o.len;
  st.skip[b] = o.skip;
  st.take[b] = o.take;
  st.t_old[b] = o.t_old;
  st.n[b] = o.n;
}

// one thread per code of the window: (row j, layer r) of slot blockIdx.y
__global__ void __launch_bounds__(256) stream_window_kernel(const StreamState st, const int32_t* __restrict__ new_codes,
                                                             int ncodes, int32_t* n_invalid) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int W = st.W, R = st.R;
  if (i >= W * R) return;
  const int j = i / R, r = i - j * R;
  const int len = min(st.len[b], W), t_old = st.t_old[b], n = st.n[b];
  int32_t v = 0;
  if (j < len) {
    const int f = t_old + n - len + j;  // the frame of window row j: 0 <= f < T
    int32_t* slot = st.ring + ((size_t)b * W + f % W) * R + r;
    if (f >= t_old) {  // appended by this step: f - t_old < n <= push
      v = new_codes[((size_t)b * st.push + (f - t_old)) * R + r];
      *slot = v;
      const int w = v < 0 ? v + ncodes : v;
      if (n_invalid && v != -1 && (w < 0 || w >= ncodes)) atomicAdd(n_invalid, 1);
    } else {
      v = *slot;
    }
  }
  st.window[((size_t)b * W + j) * R + r] = v;
}

// one thread per 4 samples of the slot's output
__global__ void __launch_bounds__(256) stream_emit_kernel(const StreamState st, float* __restrict__ out,
                                                           int* __restrict__ n_out) {
  const int b = blockIdx.y;
  const int u = blockIdx.x * blockDim.x + threadIdx.x;
  const int per = st.hop / 4;  // 16-byte units per frame
  const int cap = (st.push + st.halo) * per;
  const int skip = max(st.skip[b], 0);
  const int take = max(0, min(min(st.take[b], st.push + st.halo), st.W - skip));
  if (u < cap) {
    f32x4s v = {0.f, 0.f, 0.f, 0.f};
    if (u < take * per)
      v = *reinterpret_cast<const f32x4s*>(st.wav + ((size_t)b * st.W + skip) * st.hop + (size_t)u * 4);
    *reinterpret_cast<f32x4s*>(out + (size_t)b * cap * 4 + (size_t)u * 4) = v;
  }
  if (u == 0) {
    n_out[b] = take;
    st.T[b] = st.T_next[b];
    st.E[b] = st.E_next[b];
    st.closed[b] = st.closed_next[b];
  }
}

static bool stream_geometry_ok(const StreamState& st) {
  return st.sessions >= 1 && st.sessions <= kStreamMaxSessions && st.push >= 1 && st.push <= kStreamMaxFrames &&
         st.halo >= 0 && st.halo <= kStreamMaxFrames && st.R >= 1 && st.hop >= 4 && st.hop % 4 == 0 && st.T &&
         st.ring && st.window && st.wav;
}

hipError_t launch_stream_reset(const StreamState& st, hipStream_t s) {
  if (!stream_geometry_ok(st)) return hipErrorInvalidValue;
  return launch_zero_words(st.T, (long long)kStreamCounters * st.sessions, s);  // the counter arrays are contiguous
}

hipError_t launch_stream_plan(const StreamState& st, const int* n_new, const int* flags, hipStream_t s) {
  if (!stream_geometry_ok(st) || !n_new || !flags) return hipErrorInvalidValue;
  hipLaunchKernelGGL(stream_plan_kernel, dim3((st.sessions + 255) / 256), dim3(256), 0, s, st, n_new, flags);
  return hipGetLastError();
}

hipError_t launch_stream_window(const StreamState& st, const int32_t* new_codes, int ncodes, int32_t* n_invalid,
                                hipStream_t s) {
  if (!stream_geometry_ok(st) || !new_codes || ncodes < 1) return hipErrorInvalidValue;
  const unsigned gx = (unsigned)(((long long)st.W * st.R + 255) / 256);
  hipLaunchKernelGGL(stream_window_kernel, dim3(gx, st.sessions), dim3(256), 0, s, st, new_codes, ncodes, n_invalid);
  return hipGetLastError();
}

hipError_t launch_stream_emit(const StreamState& st, float* out, int* n_out, hipStream_t s) {
  if (!stream_geometry_ok(st) || !out || !n_out || (reinterpret_cast<uintptr_t>(out) & 15)) return hipErrorInvalidValue;
  const unsigned gx = (unsigned)(((long long)(st.push + st.halo) * (st.hop / 4) + 255) / 256);
  hipLaunchKernelGGL(stream_emit_kernel, dim3(gx, st.sessions), dim3(256), 0, s, st, out, n_out);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Audio streams (dcx_stream_encode_step; DESIGN.md §3 "Audio streams"): the same three kernels around
// the slot tokenization of one step.
//  * audio_stream_plan: audio_plan_step per slot;
//  * audio_stream_window: the step's samples appended to the sample ring (raw sample r at r % Ws) and the
//    slot's window, raw samples [start, M), from the ring and the appended samples.  A window is at
//    most Ws consecutive samples, so the ring positions read (samples below the old M) and written
//    (from it on) are distinct.  start and Ws are multiples of 4, so a window unit of 4 samples that
//    lies in the ring is one 16-byte copy; the appended samples start anywhere in the ring, so they
//    are 16-byte where both sides are aligned;
//  * audio_stream_emit: the emitted rows of the window's codes (and x_pjt_in), -1 (zeros) behind
//    them, and the commit of the counters.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) audio_stream_plan_kernel(const AudioStreamState st, const int* __restrict__ n_new,
                                                                 const int* __restrict__ flags) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= st.sessions) return;
  AudioSlot s{st.M[b], st.C[b], st.closed[b]};
  const AudioStep o = audio_plan_step(st.geo, st.halo, st.push, s, n_new[b], flags[b]);
  st.M_next[b] = s.M;
  st.C_next[b] = s.C;
  st.closed_next[b] = s.closed;
  st.len[b] = o.len;
  st.start[b] = o.start;
  st.skip[b] = o.skip;
  st.take[b] = o.take;
  st.m_old[b] = o.m_old;
  st.n[b] = o.n;
}

// one thread per 4 samples: unit u of the slot's ring (the append) and of its window (the copy)
__global__ void __launch_bounds__(256) audio_stream_window_kernel(const AudioStreamState st,
                                                                   const float* __restrict__ new_samples) {
  const int b = blockIdx.y;
  const int j0 = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
  const int Ws = st.Ws;
  if (j0 >= Ws) return;
  const int m_old = st.m_old[b], n = min(max(st.n[b], 0), st.push);
  const int start = st.start[b], len = min(max(st.len[b], 0), min(Ws, m_old + n - start));
  float* ring = st.ring + (size_t)b * Ws;
  const float* nw = new_samples + (size_t)b * st.push;
  {  // ring positions j0 .. j0 + 3 hold appended samples i0 .. (mod Ws) where those lie below n
    const int r0 = m_old % Ws;
    const int i0 = j0 >= r0 ? j0 - r0 : j0 - r0 + Ws;
    if (i0 <= n - 4) {  // no wrap inside the unit: i0 + 3 < n <= Ws
      f32x4s v;
      if ((reinterpret_cast<uintptr_t>(nw + i0) & 15) == 0) v = *reinterpret_cast<const f32x4s*>(nw + i0);
      else v = f32x4s{nw[i0], nw[i0 + 1], nw[i0 + 2], nw[i0 + 3]};
      *reinterpret_cast<f32x4s*>(ring + j0) = v;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int i = i0 + e >= Ws ? i0 + e - Ws : i0 + e;
        if (i < n) ring[j0 + e] = nw[i];
      }
    }
  }
  f32x4s w = {0.f, 0.f, 0.f, 0.f};
  if (j0 + 3 < len && start + j0 + 3 < m_old) {
    w = *reinterpret_cast<const f32x4s*>(ring + (start + j0) % Ws);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int p = start + j0 + e;  // < M = m_old + n where j0 + e < len
      if (j0 + e < len) w[e] = p < m_old ? ring[p % Ws] : nw[p - m_old];
    }
  }
  *reinterpret_cast<f32x4s*>(st.window + (size_t)b * Ws + j0) = w;
}

// one thread per code of the output, and per 4 values of its x_pjt_in rows
__global__ void __launch_bounds__(256) audio_stream_emit_kernel(const AudioStreamState st, int32_t* __restrict__ codes_out,
                                                                 int* __restrict__ n_out, float* __restrict__ pin_out) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int K = st.K, R = st.R, Wf = st.Wf;
  const int skip = min(max(st.skip[b], 0), Wf);
  const int take = max(0, min(min(st.take[b], K), Wf - skip));
  if (i < K * R) {
    const int k = i / R, r = i - k * R;
    codes_out[((size_t)b * K + k) * R + r] = k < take ? st.codes[((size_t)b * Wf + skip + k) * R + r] : -1;
  }
  if (pin_out) {
    const int per = st.CD / 4;
    if (i < K * per) {
      const int k = i / per, c = (i - k * per) * 4;
      f32x4s v = {0.f, 0.f, 0.f, 0.f};
      if (k < take) v = *reinterpret_cast<const f32x4s*>(st.pin + ((size_t)b * Wf + skip + k) * st.CD + c);
      *reinterpret_cast<f32x4s*>(pin_out + ((size_t)b * K + k) * st.CD + c) = v;
    }
  }
  if (i == 0) {
    n_out[b] = take;
    st.M[b] = st.M_next[b];
    st.C[b] = st.C_next[b];
    st.closed[b] = st.closed_next[b];
  }
}

static bool audio_stream_geometry_ok(const AudioStreamState& st) {
  return st.sessions >= 1 && st.sessions <= kStreamMaxSessions && st.push >= 1 && st.push <= kAudioStreamMaxPush &&
         st.halo >= 0 && st.halo <= kStreamMaxFrames && st.R >= 1 && st.geo.hop >= 4 && st.geo.hop % 4 == 0 &&
         st.Ws >= st.push && st.Ws % st.geo.hop == 0 && st.Wf == st.Ws / st.geo.hop && st.K >= 1 && st.CD >= 0 &&
         st.CD % 4 == 0 && st.M && st.ring && st.window && st.codes && (st.CD == 0 || st.pin);
}

hipError_t launch_audio_stream_reset(const AudioStreamState& st, hipStream_t s) {
  if (!audio_stream_geometry_ok(st)) return hipErrorInvalidValue;
  return launch_zero_words(st.M, (long long)kAudioStreamCounters * st.sessions, s);  // contiguous arrays
}

hipError_t launch_audio_stream_plan(const AudioStreamState& st, const int* n_new, const int* flags, hipStream_t s) {
  if (!audio_stream_geometry_ok(st) || !n_new || !flags) return hipErrorInvalidValue;
  hipLaunchKernelGGL(audio_stream_plan_kernel, dim3((st.sessions + 255) / 256), dim3(256), 0, s, st, n_new, flags);
  return hipGetLastError();
}

hipError_t launch_audio_stream_window(const AudioStreamState& st, const float* new_samples, hipStream_t s) {
  if (!audio_stream_geometry_ok(st) || !new_samples) return hipErrorInvalidValue;
  const unsigned gx = (unsigned)((st.Ws / 4 + 255) / 256);
  hipLaunchKernelGGL(audio_stream_window_kernel, dim3(gx, st.sessions), dim3(256), 0, s, st, new_samples);
  return hipGetLastError();
}

hipError_t launch_audio_stream_emit(const AudioStreamState& st, int32_t* codes_out, int* n_out, float* pin_out,
                                    hipStream_t s) {
  if (!audio_stream_geometry_ok(st) || !codes_out || !n_out || (pin_out && (!st.pin || (reinterpret_cast<uintptr_t>(pin_out) & 15))))
    return hipErrorInvalidValue;
  const long long items = std::max((long long)st.K * st.R, pin_out ? (long long)st.K * (st.CD / 4) : 0LL);
  hipLaunchKernelGGL(audio_stream_emit_kernel, dim3((unsigned)((items + 255) / 256), st.sessions), dim3(256), 0, s, st,
                     codes_out, n_out, pin_out);
  return hipGetLastError();
}

}  // namespace dcx
