// Internal header of the host runtime behind include/distilcodec_amd.h: the handle, the activation
// and workspace types, the error / launch macros, and what the host units call across files.
// Only the host .cpp files include it, never a .hip file (DESIGN.md has the file map).
//
// Stage call graphs follow the reference modules (paths under the reference checkout):
//   mel      mel_spec.py:26-57,100-122
//   encode   encoders.py:68-76, convnext_utils.py:186-282
//   vq       grfvq.py:105-146, residual_vq.py:103-259, vector_quantize_pytorch.py:41-45,462-538
//   generate generators.py:118-147, convnext_utils.py:106-113,137-138
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../../include/distilcodec_amd.h"
#include "dcx_kernels.h"

using dcx::ConvParams;

namespace dcx::host {

struct HostTensor {
  std::vector<int64_t> shape;
  std::vector<float> data;
  int64_t numel() const {
    int64_t n = 1;
    for (auto s : shape) n *= s;
    return n;
  }
};

struct ConvW {
  float* w = nullptr;
  unsigned short* w6 = nullptr;  // bf16 3-plane split, x6 kernel layout
  unsigned short* wc = nullptr;  // 1x1 convs: hi plane only, [Cin/32][Cout][32] (bf16 mode, conv_gemm_bf16dm)
  unsigned short* w3 = nullptr;  // h3 arithmetic: fp16 h / l of w * 2^w3_shift (ConvParams::w3)
  int w3_shift = 0;
  float* b = nullptr;
  float* b16 = nullptr;  // the bias rounded to bf16 (bf16 mode: autocast casts it with the weight)
  int cin = 0, cout = 0, taps = 1, phases = 1, in_step = 1, out_mul = 1;
  int in_base[dcx::kMaxPhases] = {0};
  // h3 activation range (round 6, dcx_kernels.h h2_shift): |out| <= g_abs max|in| + b_abs, g_abs the
  // largest absolute row sum of the weights over (phase, output channel), b_abs = max |bias|
  float g_abs = 0.f, b_abs = 0.f;
};

struct LnW {
  float* w = nullptr;
  float* b = nullptr;
  int C = 0;
};

struct BlockW {  // ConvNeXtBlock
  int C = 0;
  float *dww = nullptr, *dwb = nullptr, *gamma = nullptr;
  LnW ln;
  ConvW pw1, pw2;
};

struct ProfRec {
  int id;
  int ev0, ev1;
  double flops, bytes;
};

struct Bump {  // workspace carve-out, 256-byte aligned
  char* base;
  size_t cap, off = 0;
  bool dry;
  Bump(void* p, size_t c, bool d) : base((char*)p), cap(c), dry(d) {}
  float* f(size_t n) { return (float*)raw(n * sizeof(float)); }
  int* i(size_t n) { return (int*)raw(n * sizeof(int)); }
  unsigned short* u16(size_t n) { return (unsigned short*)raw(n * sizeof(unsigned short)); }
  void* raw(size_t bytes) {
    size_t o = (off + 255) & ~(size_t)255;
    off = o + bytes;
    return dry ? nullptr : base + o;
  }
  bool ok() const { return off <= cap; }
};

}  // namespace dcx::host

// the handle and the C ABI live in the global namespace
using namespace dcx::host;

struct dcx_codec {
  dcx_config cfg;
  int device = 0;
  std::string err;
  std::map<std::string, HostTensor> host;
  bool finalized = false, has_gen = false;
  std::vector<void*> allocs;

  ConvW dft, melfb;
  ConvW stem;
  // one-tap views of the DFT and the stem for ragged batches (dcx_tokenize_ragged): the same packed
  // weights read as [Cout][taps * Cin] (every packing is tap-major), over whole frames / unfolded rows
  ConvW dft1, stem1;
  LnW stem_ln, enc_norm;
  LnW ds_ln[4];
  ConvW ds_conv[4];
  std::vector<BlockW> blocks[4];

  ConvW vq_down, vq_pin, vq_up;
  BlockW vq_down_blk, vq_up_blk;
  int* rflag = nullptr;  // device RangeFlag bits (dcx_range_flags; round 6)
  // the residual chain (dcx_set_num_codebooks; residual_vq.py:140-259): layer k quantizes what layer
  // k - 1 left over, each with its own codebook and search bounds; project_in / project_out are shared
  int n_layers = 1;
  struct VqLayer {
    float *codebook = nullptr, *e2 = nullptr;
    double* e2d = nullptr;          // |e|^2 per code in fp64 (the rescore)
    float emax = 0.f, e2max = 0.f;  // largest codebook row norm / squared norm (prefilter bound)
    float dmax = 0.f;               // largest |e - bf16(e)| over the codes (vq_prefilter_b1's bound)
    unsigned short* codebook6 = nullptr;
    unsigned short* codebook_b1 = nullptr;  // [CD/32][NC][32] bf16 hi (vq_prefilter_b1)
  } vq[DCX_MAX_CODEBOOKS];
  // project_out, live for the chain's decode (gather-sum, then this 1x1 conv: the reference's order) and
  // the module hook; one codebook decodes through the tables below instead
  ConvW vq_pout;
  float* ptable = nullptr;
  int* vq_stats = nullptr;        // [rows rescored, codes rescored] (dcx_vq_rescore_stats)
  bool vq_stats_on = false;       // counted from the first dcx_vq_rescore_stats call on
  unsigned short* ptable6 = nullptr;  // decode table as activation planes (x6 mode gathers)
  // bf16-mode decode table (planes; mid = lo = 0): project_out under autocast, bf16(bf16(E) W16^T + b16)
  unsigned short* ptable6b = nullptr;
  int gemm_mode = DCX_GEMM_X6;
  // fused ResBlock pairs for the C = 32 / 64 generator stages (conv_res_pair); DCX_NO_RESPAIR=1 at
  // dcx_create keeps the per-conv launches (A/B comparisons)
  bool res_pair = true;
  // compact bf16 activations between bf16-mode producers and conv_gemm_bf16dm, and x_pjt_in for vq_prefilter_b1;
  // DCX_NO_COMPACT=1 at dcx_create keeps the planes layout (A/B comparisons, same bits)
  bool compact = true;
  // rescore candidate-list capacity per searched row (VqScratch); DCX_VQ_PAIRS_PER_ROW at dcx_create
  // (0: every uncertified row is rescored in place, the overflow path; tests)
  int vq_pairs_per_row = 128;
  // split-K latency mode (dcx_set_split_k): at most split_k K-slices per few-tile x6 conv; the
  // partial sums live in the first kSplitScratch bytes of each stage call's workspace.  split_buf
  // points there only for the duration of one stage call (CallScope), which `busy` makes exclusive.
  // One region per call, so one stream per call: no half-batch fork in this mode (may_fork).
  int split_k = 0;
  float* split_buf = nullptr;
  // A/B and test switches, read from the environment once at dcx_create (knobs_from_env) and changed
  // only by dcx_set_knob; every launcher gets them through its parameters
  dcx::Knobs knobs;
  std::atomic<int> busy{0};
  // a second stream for the encoder's second half-batch (stage_encode), forked from and joined to
  // the caller's stream by events; created at dcx_finalize on the handle's device
  hipStream_t side = nullptr;
  hipEvent_t fork_ev = nullptr, join_ev = nullptr;

  ConvW conv_pre;
  ConvW ups[8];
  ConvW res[8][4][4][2];
  float* post_w = nullptr;
  float post_b = 0.f;

  const char* last_kname = "";  // the kernel run_conv launched last (dcx_conv_last_kernel)

  bool prof = false;
  std::vector<hipEvent_t> events;
  int ev_used = 0;
  std::vector<ProfRec> pending;
  std::vector<std::string> prof_names;
  std::map<std::string, int> prof_ids;
  std::vector<int64_t> prof_launches;
  std::vector<double> prof_ms, prof_flops, prof_bytes;
};

namespace dcx::host {

inline int fail(dcx_codec* h, int code, const std::string& m) {
  if (h) h->err = m;
  return code;
}

#define HIPCHK(h, expr)                                                                   \
  do {                                                                                    \
    hipError_t e_ = (expr);                                                               \
    if (e_ != hipSuccess)                                                                 \
      return fail(h, DCX_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));     \
  } while (0)

#define RUN(expr)             \
  do {                        \
    int rc_ = (expr);         \
    if (rc_ != DCX_OK) return rc_; \
  } while (0)

// After a stage body has carved its buffers from ws: a dry run (sizing) ends there, a real call
// goes on only if they fit.  msg: the site's error text.
#define WS_READY(h, ws, msg)                                       \
  do {                                                             \
    if ((ws).dry) return DCX_OK;                                   \
    if (!(ws).ok()) return fail(h, DCX_ERR_WORKSPACE, msg);        \
  } while (0)

#define LAUNCH(h, s, name, flops, bytes, expr) \
  do {                                         \
    ProfScope ps_(h, s);                       \
    HIPCHK(h, expr);                           \
    ps_.done(name, flops, bytes);              \
  } while (0)

// ----------------------------------------------------------------------------------------
// profiling
// ----------------------------------------------------------------------------------------
inline int prof_event(dcx_codec* h) {
  if (h->ev_used == (int)h->events.size()) {
    hipEvent_t e;
    if (hipEventCreate(&e) != hipSuccess) return -1;
    h->events.push_back(e);
  }
  return h->ev_used++;
}

struct ProfScope {
  dcx_codec* h;
  hipStream_t s;
  int e0 = -1;
  ProfScope(dcx_codec* h_, hipStream_t s_) : h(h_), s(s_) {
    if (h->prof) {
      e0 = prof_event(h);
      if (e0 >= 0) hipEventRecord(h->events[e0], s);
    }
  }
  void done(const char* name, double flops, double bytes) {
    if (!h->prof || e0 < 0) return;
    int e1 = prof_event(h);
    if (e1 < 0) return;
    hipEventRecord(h->events[e1], s);
    auto it = h->prof_ids.find(name);
    int id;
    if (it == h->prof_ids.end()) {
      id = (int)h->prof_names.size();
      h->prof_ids[name] = id;
      h->prof_names.push_back(name);
      h->prof_launches.push_back(0);
      h->prof_ms.push_back(0);
      h->prof_flops.push_back(0);
      h->prof_bytes.push_back(0);
    } else {
      id = it->second;
    }
    h->pending.push_back({id, e0, e1, flops, bytes});
  }
};

inline unsigned short bf16_rne(float x) {
  unsigned u;
  std::memcpy(&u, &x, 4);
  return (unsigned short)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}
inline float bf16_f(unsigned short b) {
  unsigned u = (unsigned)b << 16;
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}

// An activation tensor [rows][C]: fp32 (f) and/or its 16-bit image (p) in the layout lay
// (dcx_kernels.h Layout).
// Range of a tensor (round 6, dcx_kernels.h h2_shift): in the h2 layout it holds x * 2^ash[clip]
// (ash null: ash_c for every clip); |x| <= max(amax[clip], amax_f) (amax null: amax_f), the input
// term of its consumers' bound programs.
// ash_row (one-tap consumers): a shift per row instead.
struct Rng {
  const int* ash = nullptr;
  int ash_c = 0;
  const float* amax = nullptr;
  float amax_f = 0.f;
  const int* ash_row = nullptr;
};
struct Act {
  float* f = nullptr;
  unsigned short* p = nullptr;
  Layout lay = LAYOUT_PLANES;
  Rng r;
  // per-row range buffers an h2 producer fills for a one-tap consumer (round 6): the shift and (for
  // LayerNorm outputs) the max |.| of each row
  int* row_ash = nullptr;
  float* row_amax = nullptr;
};
// the layout of a tensor whose consumer runs in h3 arithmetic (h2) or in x6 (planes)
inline Layout h2_if(bool h3) { return h3 ? LAYOUT_H2 : LAYOUT_PLANES; }
struct CAct {
  const float* f = nullptr;
  const unsigned short* p = nullptr;
  Layout lay = LAYOUT_PLANES;
  Rng r;
  CAct() = default;
  CAct(const float* f_, const unsigned short* p_, Layout lay_ = LAYOUT_PLANES) : f(f_), p(p_), lay(lay_) {}
  CAct(const Act& a) : f(a.f), p(a.p), lay(a.lay), r(a.r) {}
};

// planes layout for every GEMM operand (x6 and bf16 modes)
inline bool x6_mode(const dcx_codec* h) { return h->gemm_mode != DCX_GEMM_F32; }

struct ConvCall {
  CAct x;
  long long x_bstride;
  int batch, Lin, Lq, ldx;
  float* y = nullptr;            // v
  float* y2 = nullptr;           // silu(v), fp32
  unsigned short* y6 = nullptr;  // image of v, in y_lay (out_to)
  unsigned short* y6s = nullptr; // image of silu(v), in ys_lay: planes or h2 (silu_to)
  Layout y_lay = LAYOUT_PLANES, ys_lay = LAYOUT_PLANES;
  float* macc = nullptr;
  const float* res = nullptr;
  const float* gamma = nullptr;
  int epi = dcx::EPI_BIAS, mean = dcx::MEAN_NONE;
  bool exact = false;  // keep x6 arithmetic in bf16 mode (the reference's fp32 mel front end)
  bool silu_in = false;  // fp32 input: the conv consumes silu(x) (applied while staging)
  bool fixed_tiles = false;  // ConvParams::fixed_tiles: the kernel family does not follow the row count
  // h3 range (round 6): the bound program of an h2 output, where its per-clip shift goes, and where
  // the per-clip max |v| of the output goes (ConvParams::yb / y_ash / y_amax)
  dcx::RangeProg yb{};
  int* y_ash = nullptr;
  float* y_amax = nullptr;
  // ragged batch (ConvParams::clip_len): per-clip frame counts in device memory and this conv's
  // output rows (per phase) per frame; the launch's shape stays the padded one
  const int* lens = nullptr;
  int len_mul = 1;
  void ragged(const int* l, int frames_max) {
    lens = l;
    len_mul = l ? Lq / frames_max : 1;
  }
  void silu_to(const Act& a) {
    y2 = a.f;
    y6s = a.p;
    ys_lay = a.lay;
  }
  void out_to(const Act& a) { y = a.f; y6 = a.p; y_lay = a.lay; }
};

// Per-call range slots of the generator (round 6): measured per-clip maxima and h2 shifts, [slot][clip],
// zeroed once at the start of the call (one memset; capture-safe).
struct RangeArena {
  float* base = nullptr;
  int batch = 0, used = 0;
  static constexpr int kSlots = 320;
  void reserve(Bump& ws, int b) {
    batch = b;
    base = ws.f((size_t)kSlots * b);
  }
  // h3 range slots are only consumed by h2 tensors; a call past the capacity fails loudly
  float* amax() { return used < kSlots && base ? base + (size_t)(used++) * batch : nullptr; }
  int* ash() { return reinterpret_cast<int*>(amax()); }
  bool ok() const { return used < kSlots; }
};

// split-K latency mode (dcx_dispatch.cpp): the partial sums' scratch at the head of a call's workspace
constexpr long long kSplitMaxOut = 1LL << 21;        // floats per partial output (8 MiB)
constexpr int kSplitMax = 16;
constexpr size_t kSplitScratch = (size_t)kSplitMax * kSplitMaxOut * sizeof(float);

// workspace of one nearest-code search (vq_scratch, run_vq_search: dcx_stages.cpp)
struct VqScratch {
  float *x2 = nullptr, *xr2 = nullptr, *pv = nullptr, *pv2 = nullptr;
  int* pi = nullptr;
  double *x2d = nullptr, *cdist = nullptr;
  int* ccode = nullptr;
  int2 *pairs = nullptr, *row_list = nullptr;
  unsigned long long* npairs = nullptr;
  long long cap = 0;
};

// Buffers of one generator stage's ParallelBlock (run_parallel_block).
struct PBlockBufs {
  float* X = nullptr;                // ConvT output: the ResBlocks' input (fp32)
  Act XS;                            // silu(X) in the c1 convs' input form (unused when silu is applied on load)
  float* R[dcx::kMaxGroup] = {};     // ResBlock states (fp32)
  Act RS[dcx::kMaxGroup];            // silu(R), c1 input form
  Act Tb[dcx::kMaxGroup];            // silu(c1 output) buffers as allocated
  Act Tb_in[dcx::kMaxGroup];         // the same in the c2 convs' input form
  float* Mx = nullptr;               // mean accumulator; silu(mean) in fp32 when `last`
  Act next;                          // silu(mean) in the next ConvT's input form (not `last`)
  bool last = false;
  // h3 ranges (round 6): the measured per-clip max |X| (XS.r carries its h2 shift), the slots that
  // receive the mean's max |.| and h2 shift (not `last`), and the call's slots for everything else
  const float* amax_X = nullptr;
  float* next_amax = nullptr;
  int* next_ash = nullptr;
  RangeArena* ra = nullptr;
  // ragged batch (stage_generate): per-clip frame counts (device) and the padded frame count
  const int* lens = nullptr;
  int frames_max = 0;
};

// ---- dcx_weights.cpp ----
float round_up(double v);
int build_weights(dcx_codec* h, bool dry, int32_t with_generator);
int build_conv(dcx_codec* h, int cin, int cout, int k, int dilation, bool transposed, int stride, ConvW& w);

// ---- dcx_dispatch.cpp ----
void prog_add(dcx::RangeProg& p, float g, const Rng& r);
dcx::RangeProg prog_conv(const ConvW& w, const Rng& in);
Act conv_input(dcx_codec* h, Bump& ws, size_t n);
bool f32_input_ok(const ConvW& w);
int dcx::Knobs::*knob_slot(const std::string& n);
void knobs_from_env(dcx::Knobs& k);
int conv_params(dcx_codec* h, const ConvW& w, const ConvCall& c, bool force_f32, ConvParams& p);
bool takes_compact(const dcx_codec* h, const ConvW& w, long long rows);
bool takes_h3_conv(const dcx_codec* h, const ConvW& w, long long rows);
bool takes_h3(const dcx_codec* h, const ConvW& w);
Layout input_layout(const dcx_codec* h, const ConvW& w, long long rows, bool h3_ranges = true);
bool h3_rows_ok(long long rows, int cin);
double conv_flops(const ConvW& w, const ConvCall& c);
double conv_bytes(const ConvW& w, const ConvCall& c);
int run_conv(dcx_codec* h, const ConvW& w, const ConvCall& c, hipStream_t s, bool force_f32 = false);
int run_conv_group_split(dcx_codec* h, const ConvW* const* w, const ConvCall* c, ConvParams* p, int n, double fl,
                         double by, hipStream_t s);
int run_conv_group(dcx_codec* h, const ConvW* const* w, const ConvCall* c, int n, hipStream_t s);
ConvCall pointwise(CAct x, long long rows);
ConvCall framed(CAct x, int B, int L, int C);
int ensure_planes(dcx_codec* h, CAct& a, long long rows, int C, Bump& ws, hipStream_t s,
                  Layout want = LAYOUT_PLANES, int clips = 0, const int* lens = nullptr);
int run_block(dcx_codec* h, const BlockW& bw, float* x, unsigned short* out6, int B, int T, Act ln, Act hid,
              hipStream_t s, Layout out_lay = LAYOUT_PLANES, const dcx::RaggedSeg* rg = nullptr);
int run_ln(dcx_codec* h, const LnW& l, const float* x, Act y, long long rows, hipStream_t s, bool bf16_in = false);
void row_ranges(dcx_codec* h, Bump& ws, long long M, Act& ln, Act& hid);

// ---- dcx_stages.cpp ----
int64_t frames_of(const dcx_config& c, int64_t n);
int stage_mel(dcx_codec* h, const float* audio, int B, int64_t n, Act mel, Bump& ws, hipStream_t s,
              float* loglin = nullptr);
// fork: the call may put its second half-batch on the side stream (false inside a half of stage_encode_decode)
int stage_encode(dcx_codec* h, CAct mel, int B, int T, Act feat, Bump& ws, hipStream_t s,
                 const dcx::RaggedSeg* rg = nullptr, bool fork = true);
Layout vq_xlayout(const dcx_codec* h);
VqScratch vq_scratch(const dcx_codec* h, Bump& ws, long long M, int ntiles, bool x6);
// layer: whose codebook; x_bf16: the rows of P are bf16 values (layer 0 in bf16 mode); have_norms: the
// caller has filled v.x2 / x2d / xr2 and zeroed v.npairs (vq_residual_step), so row_sqnorm is skipped
int run_vq_search(dcx_codec* h, int layer, const float* P, const unsigned short* P6, Layout xl, long long M,
                  const VqScratch& v, int ntiles, int32_t* codes, hipStream_t s, bool x_bf16, bool have_norms = false);
int stage_vq_encode(dcx_codec* h, CAct feat, int B, int T, int32_t* codes, float* pin, float* fup, float* quant,
                    Bump& ws, hipStream_t s, const dcx::RaggedSeg* rg = nullptr);
// lens (ragged batches; device, [B]): codes at or beyond a clip's length are neither read nor counted,
// and the up block's depthwise conv sees zeros there, as the clip's own padding
int stage_vq_decode(dcx_codec* h, const int32_t* codes, int B, int T, Act z, int32_t* n_invalid, Bump& ws,
                    hipStream_t s, const int* lens = nullptr);
int tokenize_ragged_rows(dcx_codec* h, const float* audio, const dcx::RaggedSeg& rg, int32_t* codes, float* pin,
                         float* fup, Bump& ws, hipStream_t s);
int stage_encode_decode(dcx_codec* h, const float* audio, int B, int64_t n, int32_t* codes, float* wav, Bump& ws,
                        hipStream_t s);
int stage_decode_ragged(dcx_codec* h, const int32_t* codes, const int* lens, int B, int T, float* wav,
                        int32_t* n_invalid, Bump& ws, hipStream_t s);
// one step of a token stream on the state st views: n_invalid counts the codes the step appends
int tokenize_slots_rows(dcx_codec* h, const float* audio, const dcx::RaggedSeg& rg, int32_t* codes, float* pin, Bump& ws,
                        hipStream_t s);
int stage_audio_stream_step(dcx_codec* h, const dcx::AudioStreamState& st, const dcx::RaggedSeg& rg,
                            const float* new_samples, const int* n_new, const int* flags, int32_t* codes_out, int* n_out,
                            float* pin_out, Bump& ws, hipStream_t s);
int stage_stream_step(dcx_codec* h, const dcx::StreamState& st, const int32_t* new_codes, const int* n_new,
                      const int* flags, float* wav_out, int* n_out, int32_t* n_invalid, Bump& ws, hipStream_t s);

// ---- dcx_generator.cpp ----
bool h3_stage(const dcx_codec* h, int i, long long rows);
int run_parallel_block(dcx_codec* h, int i, int B, int Lo, const PBlockBufs& b, hipStream_t s);
Act fp32_form(dcx_codec* h, const Act& a, const ConvW& consumer);
int run_conv_post(dcx_codec* h, const float* x, float* wav, int B, int L, int C, hipStream_t s,
                  const int* lens = nullptr, int len_mul = 1);
// lens (ragged batches; device, [B] frame counts): every kernel bounds clip b by lens[b]; the kernel
// families, tiles and workspace plan follow B and T (the padded frame count) alone
int stage_generate(dcx_codec* h, CAct z, int B, int T, float* wav, Bump& ws, hipStream_t s,
                   const int* lens = nullptr);

// ---- dcx_module.cpp ----
bool module_io(const dcx_codec* h, const std::string& m, int& cin, int& cout, int& rate);
int stage_module(dcx_codec* h, const std::string& m, const float* x, int B, int L, void* yv, Bump& ws, hipStream_t s);

}  // namespace dcx::host
