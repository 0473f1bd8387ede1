// Conv dispatch of the host runtime: range programs, the A/B knobs, ConvParams of a call, the layout
// predicates, the split-K latency mode, grouped launches, the ConvNeXt block and the LayerNorm.
#include "dcx_host.h"

namespace dcx::host {

// bound programs (dcx::RangeProg): c + sum of g * max(measured, floor) terms
void prog_add(dcx::RangeProg& p, float g, const Rng& r) {
  p.m[p.n] = r.amax;
  p.g[p.n] = g;
  p.f[p.n] = r.amax_f;
  ++p.n;
}
// |conv(x) + bias| <= g_abs max|x| + b_abs (|silu(v)|, |gelu(v)| <= |v|)
dcx::RangeProg prog_conv(const ConvW& w, const Rng& in) {
  dcx::RangeProg p{};
  p.c = w.b_abs;
  prog_add(p, w.g_abs, in);
  return p;
}
// per-row bound of a one-tap conv's output from its input rows' maxima (rowwise program)
static dcx::RangeProg prog_conv_rows(const ConvW& w, const float* in_row_amax) {
  dcx::RangeProg p{};
  p.rowwise = 1;
  p.c = w.b_abs;
  p.m[0] = in_row_amax;
  p.g[0] = w.g_abs;
  p.n = 1;
  return p;
}

// Workspace for a tensor consumed only by convs: planes in x6 mode, fp32 otherwise.
Act conv_input(dcx_codec* h, Bump& ws, size_t n) {
  Act a;
  if (x6_mode(h)) a.p = ws.u16(3 * n);
  else a.f = ws.f(n);
  return a;
}

// Planes-mode convs with Cout <= 64, Cin <= 128 and a tap halo take an fp32 input (split while
// staging; conv_gemm_x6w8 AF32).
bool f32_input_ok(const ConvW& w) { return w.cin <= 128 && w.cout <= 64 && w.taps >= 2; }

// ---- A/B and test switches (dcx::Knobs): names are the environment variables dcx_create reads ----
static const struct {
  const char* name;
  int dcx::Knobs::*slot;
} kKnobs[] = {
    {"DCX_RP_R", &dcx::Knobs::rp_rows},                   {"DCX_RP_OLD", &dcx::Knobs::rp_old},
    {"DCX_RP_G64", &dcx::Knobs::rp_g64},                  {"DCX_GELU_LUT", &dcx::Knobs::gelu_lut},
    {"DCX_BF16_PERSIST", &dcx::Knobs::bf16_persist},      {"DCX_BF16_REG_EPI", &dcx::Knobs::bf16_reg_epi},
    {"DCX_DWCONV_TILED", &dcx::Knobs::dwconv_tiled},      {"DCX_SPLIT_MIN_STEPS", &dcx::Knobs::split_min_steps},
    {"DCX_SPLIT_GROUP_OFF", &dcx::Knobs::split_group_off}, {"DCX_H3", &dcx::Knobs::h3},
    {"DCX_H3_BN", &dcx::Knobs::h3_bn},                    {"DCX_H3_1X1", &dcx::Knobs::h3_1x1},
    {"DCX_H3_SPLIT", &dcx::Knobs::h3_split},              {"DCX_H3_PAIRS", &dcx::Knobs::h3_pairs},
    {"DCX_RP_RING", &dcx::Knobs::rp_ring},                {"DCX_ENC_STREAMS", &dcx::Knobs::enc_streams},
    {"DCX_EPI_GENERIC", &dcx::Knobs::epi_generic},        {"DCX_CONV_GROUP", &dcx::Knobs::conv_group}};

// the member a knob's name selects; null for unknown names
int dcx::Knobs::*knob_slot(const std::string& n) {
  for (const auto& k : kKnobs)
    if (n == k.name) return k.slot;
  return nullptr;
}

void knobs_from_env(dcx::Knobs& k) {
  for (const auto& kn : kKnobs) {
    const char* e = std::getenv(kn.name);
    if (e && *e) k.*kn.slot = std::atoi(e);
  }
}

int conv_params(dcx_codec* h, const ConvW& w, const ConvCall& c, bool force_f32, ConvParams& p) {
  const bool x6 = x6_mode(h) && !force_f32;
  const bool x6_f32in = x6 && !c.x.p && c.x.f && f32_input_ok(w);
  if (c.silu_in && !x6_f32in) return fail(h, DCX_ERR_STATE, "internal: silu_in needs an fp32-input conv");
  if (x6 ? ((!c.x.p && !x6_f32in) || !w.w6) : !c.x.f)
    return fail(h, DCX_ERR_STATE, "internal: conv input missing for GEMM mode");
  p = ConvParams{};
  p.x = c.x.f;
  p.x6 = x6 ? c.x.p : nullptr;
  p.w = w.w;
  p.w6 = x6 ? w.w6 : nullptr;
  const bool one = x6 && h->gemm_mode == DCX_GEMM_BF16 && !c.exact;
  p.bias = one && w.b16 ? w.b16 : w.b;  // autocast rounds the bias with the other operands
  p.gamma = c.gamma;
  p.res = c.res;
  p.y = c.y;
  p.y2 = c.y2;
  p.y6 = c.y6;
  p.y6s = c.y6s;
  p.macc = c.macc;
  p.x_bstride = c.x_bstride;
  p.ldy = w.cout;
  p.y_bstride = (long long)c.Lq * w.out_mul * p.ldy;
  p.w_phase_stride = (long long)w.cout * w.taps * w.cin;
  p.Lin = c.Lin;
  p.Lq = c.Lq;
  p.Cin = w.cin;
  p.Cout = w.cout;
  p.ldx = c.ldx ? c.ldx : w.cin;
  p.taps = w.taps;
  p.in_step = w.in_step;
  p.out_mul = w.out_mul;
  for (int i = 0; i < dcx::kMaxPhases; ++i) p.in_base[i] = w.in_base[i];
  p.epi = c.epi;
  p.mean_mode = c.mean;
  p.nprod = one ? 1 : 6;
  p.round_bf16 = one;
  p.silu_in = c.silu_in;
  p.fixed_tiles = c.fixed_tiles ? 1 : 0;
  p.x_layout = x6 && c.x.p ? c.x.lay : LAYOUT_PLANES;
  p.y_layout = c.y6 ? c.y_lay : LAYOUT_PLANES;
  p.ys_layout = c.y6s ? c.ys_lay : LAYOUT_PLANES;
  if (p.x_layout == LAYOUT_H2) {  // h3 arithmetic (conv_gemm_x3dq)
    if (!w.w3 || one) return fail(h, DCX_ERR_STATE, "internal: h2 input without h3 weights");
    p.w3 = w.w3;
    p.w3_shift = w.w3_shift;
    p.x_ash = c.x.r.ash;
    p.x_ash_c = c.x.r.ash_c;
    p.x_ash_row = c.x.r.ash_row;
    if (p.x_ash_row && (w.taps != 1 || w.phases != 1 || w.in_base[0] != 0))
      return fail(h, DCX_ERR_STATE, "internal: per-row input ranges need a one-tap conv");
  }
  p.y_ash = c.y_ash;
  p.y_amax = c.y_amax;
  p.yb = c.yb;
  p.rflag = h->rflag;
  p.clip_len = c.lens;
  p.len_mul = c.len_mul;
  if (c.lens && (c.len_mul < 1 || !x6 || one)) return fail(h, DCX_ERR_STATE, "internal: ragged conv outside x6 mode");
  p.wc = one && h->compact ? w.wc : nullptr;
  p.kn = &h->knobs;
  // compact inputs only feed one-product GEMMs; a compact output (the RNE hi value) may also be written
  // in x6 mode (x_pjt_in for vq_prefilter_b1)
  for (Layout l : {p.x_layout, p.y_layout, p.ys_layout})
    if (l != LAYOUT_PLANES && l != LAYOUT_BF16 && l != LAYOUT_H2) return fail(h, DCX_ERR_STATE, "internal: not a layout");
  if (p.ys_layout == LAYOUT_BF16) return fail(h, DCX_ERR_STATE, "internal: y6s takes planes or h2 only");
  if (p.x_layout == LAYOUT_BF16 && !one) return fail(h, DCX_ERR_STATE, "internal: compact layout outside bf16 mode");
  if (p.y_layout == LAYOUT_H2 && (!x6 || one)) return fail(h, DCX_ERR_STATE, "internal: h2 layout outside x6 mode");
  return DCX_OK;
}

// Whether a one-tap conv over `rows` rows runs on conv_gemm_bf16dm in this handle's mode, so its
// producer may write the compact bf16 layout (2 bytes per element instead of 6).
bool takes_compact(const dcx_codec* h, const ConvW& w, long long rows) {
  return h->compact && h->gemm_mode == DCX_GEMM_BF16 && w.wc && w.taps == 1 && w.phases == 1 && w.in_base[0] == 0 &&
         rows < (1LL << 31) && dcx::bf16dm_takes(w.cin, w.cout, (int)rows, w.cin, 1);
}

// The layout a producer writes for the one-tap conv w over `rows` rows: compact where conv_gemm_bf16dm
// takes it, h2 where an h3 kernel does and the producer has the row ranges (h3_ranges), else planes.
// takes_compact needs bf16 mode and takes_h3 x6 mode, so the two are never both true.
Layout input_layout(const dcx_codec* h, const ConvW& w, long long rows, bool h3_ranges) {
  return takes_compact(h, w, rows) ? LAYOUT_BF16 : h3_ranges && takes_h3(h, w) ? LAYOUT_H2 : LAYOUT_PLANES;
}

// Whether a generator conv with a tap halo (conv_pre, the ConvTs with Cout % 128 == 0) runs in h3
// arithmetic (conv_gemm_x3dw; Knobs::h3, x6 mode, not in the split-K latency mode), so its producer
// writes h2.
// The h3 tap kernels address a clip's input through one buffer descriptor: (rows + 1024) * Cin * 4
// bytes must stay under 2^31 (dcx_conv.hip x3dq_ok); longer clips (> ~11 min at the C = 256 stage)
// keep the x6 kernels, whose tiles rebase their descriptors.
bool h3_rows_ok(long long rows, int cin) { return (rows + 1024) * cin * 4LL < (1LL << 31); }

// rows: the conv's input rows per clip
bool takes_h3_conv(const dcx_codec* h, const ConvW& w, long long rows) {
  return h->knobs.h3 && h->gemm_mode == DCX_GEMM_X6 && h->split_k < 2 && w.w3 && w.taps >= 2 && w.cout % 128 == 0 &&
         h3_rows_ok(rows, w.cin);
}

// Whether a one-tap conv runs in h3 arithmetic (conv_gemm_x3dm; Knobs::h3_1x1, x6 mode, not in the
// split-K latency mode), so its producer writes the h2 layout.
bool takes_h3(const dcx_codec* h, const ConvW& w) {
  return h->knobs.h3_1x1 && h->gemm_mode == DCX_GEMM_X6 && h->split_k < 2 && w.w3 && w.taps == 1 && w.phases == 1 &&
         w.in_base[0] == 0 && w.cout % 128 == 0;
}

// algorithmic FLOPs and bytes of one conv (profiling)
double conv_flops(const ConvW& w, const ConvCall& c) { return 2.0 * c.batch * c.Lq * w.phases * w.cout * w.cin * w.taps; }
double conv_bytes(const ConvW& w, const ConvCall& c) {
  const double outs = (double)c.batch * c.Lq * w.phases * w.cout;
  return 4.0 * ((double)c.batch * c.Lin * w.cin + outs + (double)w.phases * w.cout * w.taps * w.cin);
}

// ---- split-K latency mode --------------------------------------------------------------------
// A conv whose output fits kSplitMaxOut floats and whose tiles leave most CUs idle (the few-tile
// kernels) runs as S K-slices over input-channel chunks, each writing fp32 partial sums, and one
// reduce kernel that sums them in slice order and applies the conv's epilogue.  Summation order
// (and so the low bits) then depends on S, i.e. on the tile count: the mode is opt-in and a clip
// alone is not bit-equal to the same clip in a batch.
static int split_factor(const dcx_codec* h, const ConvW& w, const ConvCall& c, const ConvParams& p) {
  if (h->split_k < 2 || !h->split_buf || p.nprod != 6 || !p.w6 || !p.x6 || p.x_layout != LAYOUT_PLANES || w.cout % 128) return 1;
  const long long out = (long long)c.batch * c.Lq * w.out_mul * w.cout;
  if (out > kSplitMaxOut || (w.cin / 16) % (w.taps % 2 ? 2 : 1)) return 1;
  // tiles of the 256 x 128 kernels the slices run on (conv_gemm_x6pp / x6lm, whatever the big-tile
  // rule would pick unsplit: in this mode the bits depend on the split anyway)
  const long long tiles = (long long)c.batch * ((c.Lq + 255) / 256) * std::max(1, w.cout / 128) * w.phases;
  if (tiles >= 128) return 1;
  // Knobs::split_min_steps (DCX_SPLIT_MIN_STEPS; A/B): convs with fewer K steps (taps x 16-channel
  // chunks) run unsplit
  if ((long long)w.taps * (w.cin / 16) < h->knobs.split_min_steps) return 1;
  const int unit = w.taps % 2 ? 2 : 1;  // chunks per slice: an even number of steps per slice
  const long long nunits = (w.cin / 16) / unit;
  return (int)std::min<long long>({(long long)std::min(h->split_k, kSplitMax), std::max<long long>(1, 256 / tiles), nunits});
}

// A conv's parameters as S K-slices: fp32 partial sums into `part`, the epilogue left to the reduce
static ConvParams kslice_params(const ConvParams& p, const ConvW& w, int S, float* part) {
  ConvParams q = p;
  q.ksplit = S;
  q.kunit = w.taps % 2 ? 2 : 1;
  q.bias = q.gamma = q.res = nullptr;
  q.macc = nullptr;
  q.y = part;
  q.y2 = nullptr;
  q.y6 = q.y6s = nullptr;
  q.epi = dcx::EPI_BIAS;
  q.mean_mode = dcx::MEAN_NONE;
  q.y_layout = LAYOUT_PLANES;
  q.round_bf16 = 0;
  q.y_ash = nullptr;  // the slices' clips are virtual; the split-K mode runs no h3 conv
  q.y_amax = nullptr;
  return q;
}

static int run_conv_split(dcx_codec* h, const ConvW& w, const ConvCall& c, const ConvParams& p, int S, hipStream_t s) {
  ProfScope ps(h, s);
  // one launch: slice sl of clip b is virtual clip sl * batch + b, its partial sums at that clip's
  // place in split_buf; then one reduce launch applies the epilogue
  const ConvParams q = kslice_params(p, w, S, h->split_buf);
  const char* kname = "conv";
  HIPCHK(h, dcx::launch_conv(q, c.batch * S, w.phases, s, &kname));
  h->last_kname = kname;
  HIPCHK(h, dcx::launch_splitk_epilogue(p, h->split_buf, S, (long long)c.batch * p.y_bstride, c.batch, w.phases, s));
  ps.done((std::string("splitk:") + kname).c_str(), conv_flops(w, c), conv_bytes(w, c));
  return DCX_OK;
}

#ifdef DCX_DIAG_DUP
// Diagnostic builds: with DCX_DIAG_DUP=1 (no stores) or 2 (no epilogue) every conv launch is preceded
// by a timing copy on the same (real) inputs that writes nothing, profiled as "diag:<kernel>", so
// kernel tables compare each launch with and without its epilogue's stores on identical data.
static int diag_dup_mode() {
  const char* e = std::getenv("DCX_DIAG_DUP");
  return e && (e[0] == '1' || e[0] == '2') ? e[0] - '0' : 0;
}
#endif

int run_conv(dcx_codec* h, const ConvW& w, const ConvCall& c, hipStream_t s, bool force_f32) {
  ConvParams p;
  RUN(conv_params(h, w, c, force_f32, p));
  const int S = force_f32 ? 1 : split_factor(h, w, c, p);
  if (S > 1 && c.lens) return fail(h, DCX_ERR_STATE, "internal: ragged conv in the split-K mode");
  if (S > 1) return run_conv_split(h, w, c, p, S, s);
#ifdef DCX_DIAG_DUP
  if (const int dm = diag_dup_mode()) {
    ConvParams q = p;
    q.diag_skip = dm;
    ProfScope pd(h, s);
    const char* kn = "conv";
    HIPCHK(h, dcx::launch_conv(q, c.batch, w.phases, s, &kn));
    pd.done((std::string("diag:") + kn).c_str(), conv_flops(w, c), conv_bytes(w, c));
  }
#endif
  ProfScope ps(h, s);
  const char* kname = "conv";
  HIPCHK(h, dcx::launch_conv(p, c.batch, w.phases, s, &kname));
  h->last_kname = kname;
  ps.done(kname, conv_flops(w, c), conv_bytes(w, c));
  return DCX_OK;
}

// Split-K latency mode, grouped (round 4): the few-tile convs of one ResBlock dilation index (all
// three split-eligible) as ONE conv launch whose members get K-slice counts in proportion to their
// K (taps x chunks), at least two each, within the CU count of workgroups, and ONE launch of their reduces, instead of
// two launches per conv (a C5 hop spent ~7 us per reduce launch, 107 of them).  Returns 1 when the
// group does not qualify (the caller splits the members one by one).
int run_conv_group_split(dcx_codec* h, const ConvW* const* w, const ConvCall* c, ConvParams* p, int n, double fl,
                         double by, hipStream_t s) {
  if (n < 2 || h->knobs.split_group_off) return 1;
  long long tiles[dcx::kMaxGroup], out[dcx::kMaxGroup], chunks[dcx::kMaxGroup];
  int S[dcx::kMaxGroup], smax[dcx::kMaxGroup];
  // a ParallelBlock's last convs (the mean folded into their epilogues) must all be split, so that
  // one reduce thread finishes every member of an element in ResBlock order
  const bool chain = p[0].mean_mode != dcx::MEAN_NONE;
  if (chain) {
    if (p[0].mean_mode != dcx::MEAN_FIRST || p[n - 1].mean_mode != dcx::MEAN_LAST) return 1;
    for (int i = 1; i < n - 1; ++i)
      if (p[i].mean_mode != dcx::MEAN_MID) return 1;
    for (int i = 1; i < n; ++i)
      if (p[i].macc != p[0].macc || c[i].Lq != c[0].Lq || w[i]->cout != w[0]->cout) return 1;
  }
  long long total = 0;
  for (int i = 0; i < n; ++i) {
    if (split_factor(h, *w[i], c[i], p[i]) < 2 || w[i]->taps < 3 || w[i]->out_mul != 1) return 1;
    tiles[i] = (long long)c[i].batch * ((c[i].Lq + 255) / 256) * (w[i]->cout / 128);
    out[i] = (long long)c[i].batch * p[i].y_bstride;
    const int unit = w[i]->taps % 2 ? 2 : 1;
    chunks[i] = (long long)w[i]->taps * (w[i]->cin / 16);
    // at most the handle's split_k slices per member (dcx_set_split_k), as split_factor allows
    smax[i] = (int)std::min<long long>(std::min(h->split_k, kSplitMax), (w[i]->cin / 16) / unit);
    // every member is split, as split_factor splits it alone: with dcx_set_split_k(2) the grouped and
    // the per-conv launches then give every conv two slices, the same partial sums and the same bits
    // (started from one slice, a tight budget left the member with the fewest chunks unsplit)
    S[i] = 2;
    if (S[i] > smax[i]) return 1;
    total += S[i] * tiles[i];
  }
  if (total > 256) return 1;  // two slices each do not fit: the caller splits the members one by one
  // K slices: repeatedly give one more slice to the member whose slices are longest, while the
  // grid stays within one workgroup per CU
  for (;;) {
    int best = -1;
    for (int i = 0; i < n; ++i)
      if (S[i] < smax[i] && total + tiles[i] <= 256 &&
          (best < 0 || chunks[i] * S[best] > chunks[best] * S[i]))
        best = i;
    if (best < 0) break;
    ++S[best];
    total += tiles[best];
  }
  long long need = 0;
  for (int i = 0; i < n; ++i) need += S[i] > 1 ? S[i] * out[i] : 0;
  if (need > kSplitMax * kSplitMaxOut) return 1;
  ProfScope ps(h, s);
  ConvParams q[dcx::kMaxGroup], r[dcx::kMaxGroup];
  const float* part[dcx::kMaxGroup];
  int rs[dcx::kMaxGroup];
  long long rstride[dcx::kMaxGroup];
  int nr = 0;
  long long off = 0;
  for (int i = 0; i < n; ++i) {
    q[i] = p[i];
    q[i].ksplit = S[i];
    if (S[i] > 1) {  // partial sums into the split buffer, the epilogue in the reduce
      q[i] = kslice_params(p[i], *w[i], S[i], h->split_buf + off);
      r[nr] = p[i];
      part[nr] = h->split_buf + off;
      rs[nr] = S[i];
      rstride[nr] = out[i];
      ++nr;
      off += S[i] * out[i];
    }
  }
  const char* kname = "conv_group";
  const hipError_t e = dcx::launch_conv_split_group(q, n, c[0].batch, s, &kname);
  if (e == hipErrorNotSupported) return 1;
  HIPCHK(h, e);
  if (nr) HIPCHK(h, dcx::launch_splitk_epilogue_group(r, part, rs, rstride, nr, c[0].batch, chain, s));
  ps.done((std::string("splitk:") + kname).c_str(), fl, by);
  return DCX_OK;
}

// n independent convs (same batch) as one grouped launch when the kernel family allows it
// (dcx::launch_conv_group), otherwise one by one; the results are the same bits either way.
int run_conv_group(dcx_codec* h, const ConvW* const* w, const ConvCall* c, int n, hipStream_t s) {
  ConvParams p[dcx::kMaxGroup];
  double fl = 0, by = 0;
  bool same = true;
  for (int i = 0; i < n; ++i) {
    RUN(conv_params(h, *w[i], c[i], false, p[i]));
    fl += conv_flops(*w[i], c[i]);
    by += conv_bytes(*w[i], c[i]);
    same = same && c[i].batch == c[0].batch && w[i]->phases == 1;
  }
  if (same && n > 1 && h->split_k >= 2) {
    const int rc = run_conv_group_split(h, w, c, p, n, fl, by, s);
    if (rc != 1) return rc;
  }
  if (same && n > 1 && h->knobs.conv_group) {
#ifdef DCX_DIAG_DUP
    if (const int dm = diag_dup_mode()) {
      ConvParams q[dcx::kMaxGroup];
      for (int i = 0; i < n; ++i) {
        q[i] = p[i];
        q[i].diag_skip = dm;
      }
      ProfScope pd(h, s);
      const char* kn = "conv_group";
      const hipError_t e = dcx::launch_conv_group(q, n, c[0].batch, s, &kn);
      if (e == hipSuccess) pd.done((std::string("diag:") + kn).c_str(), fl, by);
    }
#endif
    ProfScope ps(h, s);
    const char* kname = "conv_group";
    const hipError_t e = dcx::launch_conv_group(p, n, c[0].batch, s, &kname);
    if (e == hipSuccess) {
      ps.done(kname, fl, by);
      return DCX_OK;
    }
    if (e != hipErrorNotSupported) HIPCHK(h, e);
  }
  for (int i = 0; i < n; ++i) RUN(run_conv(h, *w[i], c[i], s));
  return DCX_OK;
}

// Pointwise conv / Linear over all B*T rows at once.
ConvCall pointwise(CAct x, long long rows) {
  ConvCall c;
  c.x = x;
  c.x_bstride = 0;
  c.batch = 1;
  c.Lin = c.Lq = (int)rows;
  c.ldx = 0;
  return c;
}
ConvCall framed(CAct x, int B, int L, int C) {
  ConvCall c;
  c.x = x;
  c.x_bstride = (long long)L * C;
  c.batch = B;
  c.Lin = c.Lq = L;
  c.ldx = C;
  return c;
}


// fp32 -> the layout `want` for a tensor handed in by the caller (x6 / bf16 modes).  LAYOUT_H2 (an h3
// consumer; a planes tensor handed in with its fp32 copy is re-split) is range-scaled (h2_shift) by the
// exact max of each clip (`clips` clips of rows / clips rows: launch_h2_ranged, the tap convs) or, with
// clips == 0, of each row (launch_h2_rows, the one-tap convs).  The scale follows from the values alone, so
// a tensor the fused pipeline would have produced in h2 itself (a LayerNorm's output) gets the same bits.
int ensure_planes(dcx_codec* h, CAct& a, long long rows, int C, Bump& ws, hipStream_t s, Layout want, int clips,
                  const int* lens) {
  const bool rh2 = want == LAYOUT_H2;
  if (rh2 && a.p && a.lay != LAYOUT_H2 && a.f) a.p = nullptr;
  if (!x6_mode(h) || a.p) return DCX_OK;
  unsigned short* p = ws.u16((size_t)rows * C * 3);
  float* am = rh2 && clips ? ws.f((size_t)clips) : nullptr;
  int* ash = rh2 ? ws.i((size_t)(clips ? clips : rows)) : nullptr;
  WS_READY(h, ws, "workspace too small");
  // a ragged batch's tensor is bounded per clip by launch_h2_ranged alone
  if (lens && !(rh2 && clips)) return fail(h, DCX_ERR_STATE, "internal: ragged tensor outside the ranged h2 split");
  if (rh2 && clips) {
    if (clips < 1 || rows % clips) return fail(h, DCX_ERR_STATE, "internal: ranged split of a ragged batch");
    LAUNCH(h, s, "h2_ranged", 0, 12.0 * rows * C,
           dcx::launch_h2_ranged(a.f, nullptr, p, clips, rows / clips, C, 0, 0.f, am, ash, h->rflag, s, lens, 1));
    a.r = Rng{};
    a.r.ash = ash;
    a.r.amax = am;
  } else if (rh2) {
    LAUNCH(h, s, "h2_rows", 0, 8.0 * rows * C, dcx::launch_h2_rows(a.f, p, rows, C, ash, s));
    a.r = Rng{};
    a.r.ash_row = ash;
  } else {
    LAUNCH(h, s, "split_planes", 0, (want == LAYOUT_BF16 ? 6.0 : 10.0) * rows * C,
           dcx::launch_split_planes(a.f, p, rows, C, want, s));
  }
  a.p = p;
  a.lay = want;
  return DCX_OK;
}

// ConvNeXtBlock in place on x [B][T][C] (fp32 residual stream); out6: optional image (planes or
// compact, out_lay) of the block output for a following conv.  ln: [M][C], hid: [M][4C] conv-input
// scratch, written compact where their consumer takes it (bf16 mode), or in h2 with per-row ranges
// (ln.row_ash / row_amax, hid.row_ash: the LayerNorm's exact row maxima, the hidden's rows bounded
// by g1 max|LN row| + max|b1|; round 6).
// rg: the rows are a ragged batch (B = 1, T = its total frames): the depthwise conv stays inside each clip.
int run_block(dcx_codec* h, const BlockW& bw, float* x, unsigned short* out6, int B, int T, Act ln, Act hid,
              hipStream_t s, Layout out_lay, const dcx::RaggedSeg* rg) {
  const long long M = (long long)B * T;
  const int C = bw.C;
  if (out6 && out_lay == LAYOUT_H2) return fail(h, DCX_ERR_STATE, "internal: a block output in h2 goes through launch_h2_rows");
  ln.lay = input_layout(h, bw.pw1, M, ln.row_ash && ln.row_amax);
  hid.lay = input_layout(h, bw.pw2, M, hid.row_ash);
  ln.r = Rng{};
  hid.r = Rng{};
  ln.r.ash_row = ln.row_ash;
  hid.r.ash_row = hid.row_ash;
  if (rg) {
    if (B != 1 || T != rg->rows) return fail(h, DCX_ERR_STATE, "internal: ragged block rows");
    LAUNCH(h, s, "dwconv_ln_ragged", 14.0 * M * C, 8.0 * M * C,
           dcx::launch_dwconv_ln_ragged(x, ln.f, ln.p, ln.lay, bw.dww, bw.dwb, bw.ln.w, bw.ln.b, *rg, C,
                                        h->gemm_mode == DCX_GEMM_BF16 ? 1 : 0, &h->knobs, s, ln.row_ash, ln.row_amax));
  } else {
    LAUNCH(h, s, "dwconv_ln", 14.0 * M * C, 8.0 * M * C,
           dcx::launch_dwconv_ln(x, ln.f, ln.p, ln.lay, bw.dww, bw.dwb, bw.ln.w, bw.ln.b, B, T, C,
                                 h->gemm_mode == DCX_GEMM_BF16 ? 1 : 0, &h->knobs, s, ln.row_ash, ln.row_amax));
  }
  ConvCall c1 = pointwise(ln, M);
  c1.out_to(hid);
  c1.epi = dcx::EPI_GELU;
  if (hid.p && hid.lay == LAYOUT_H2) {  // |GELU(v)| <= |v| <= g1 max|LN row| + max|b1|
    c1.yb = prog_conv_rows(bw.pw1, ln.row_amax);
    c1.y_ash = hid.row_ash;
  }
  RUN(run_conv(h, bw.pw1, c1, s));
  ConvCall c2 = pointwise(hid, M);
  c2.y = x;
  c2.y6 = out6;
  c2.y_lay = out_lay;
  c2.res = x;
  c2.gamma = bw.gamma;
  c2.epi = dcx::EPI_GAMMA_RES;
  RUN(run_conv(h, bw.pw2, c2, s));
  return DCX_OK;
}

// channels-first LayerNorm; bf16_in: its input is a bf16 tensor under the reference's autocast (the
// stem's, in bf16 mode), so its mean and differences are bf16 (ln_rows form 2).  An h2 output
// is scaled per row by its exact max (y.row_ash receives the shifts, y.row_amax the maxima if set).
int run_ln(dcx_codec* h, const LnW& l, const float* x, Act y, long long rows, hipStream_t s, bool bf16_in) {
  const int form = bf16_in && h->gemm_mode == DCX_GEMM_BF16 ? 2 : 1;
  if (y.p && y.lay == LAYOUT_H2 && !y.row_ash) return fail(h, DCX_ERR_STATE, "internal: h2 LayerNorm output without row ranges");
  LAUNCH(h, s, "ln_rows", 8.0 * rows * l.C, 8.0 * rows * l.C,
         dcx::launch_ln_rows(x, y.f, y.p, y.lay, l.w, l.b, rows, l.C, 1e-6f, form, s,
                             y.row_ash, y.row_amax));
  return DCX_OK;
}

// Per-row range buffers for the block scratch of M rows (x6 mode only: the h3 one-tap convs).
void row_ranges(dcx_codec* h, Bump& ws, long long M, Act& ln, Act& hid) {
  if (!x6_mode(h)) return;
  ln.row_ash = ws.i((size_t)M);
  ln.row_amax = ws.f((size_t)M);
  hid.row_ash = ws.i((size_t)M);
}

}  // namespace dcx::host
