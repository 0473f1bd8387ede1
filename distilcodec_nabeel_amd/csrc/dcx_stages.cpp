// Stage bodies of the host runtime (dry = true only sizes the workspace): mel, encoder, VQ encode /
// decode, the whole path on one or two streams, ragged batches.
#include "dcx_host.h"

namespace dcx::host {

int64_t frames_of(const dcx_config& c, int64_t n) {
  const int64_t pad = (c.win - c.hop) / 2, padr = (c.win - c.hop + 1) / 2;
  const int64_t len = n + pad + padr;
  if (len < c.n_fft) return 0;
  return (len - c.n_fft) / c.hop + 1;
}

// ---------------- stage bodies (dry=true only sizes the workspace) ----------------
// The row-wise tail of the mel front end on M STFT rows: |STFT|, the mel filterbank, log clamp.
static int mel_from_spec(dcx_codec* h, const float* spec, Act mag, long long M, Act mel, float* loglin, hipStream_t s) {
  const int nbins = h->cfg.n_fft / 2 + 1;
  LAUNCH(h, s, "spec_mag", 4.0 * M * nbins, 4.0 * M * (h->dft.cout + h->melfb.cin),
         dcx::launch_spec_mag(spec, mag.f, mag.p, loglin, M, nbins, h->melfb.cin, s));
  ConvCall cm = pointwise(mag, M);
  cm.exact = true;
  cm.out_to(mel);
  cm.epi = dcx::EPI_LOGCLAMP;
  RUN(run_conv(h, h->melfb, cm, s));
  return DCX_OK;
}

int stage_mel(dcx_codec* h, const float* audio, int B, int64_t n, Act mel, Bump& ws, hipStream_t s, float* loglin) {
  const dcx_config& c = h->cfg;
  const int T = (int)frames_of(c, n);
  const int rows = T + c.n_fft / c.hop - 1;
  Act fr = conv_input(h, ws, (size_t)B * rows * c.hop);
  float* spec = ws.f((size_t)B * T * h->dft.cout);
  Act mag = conv_input(h, ws, (size_t)B * T * h->melfb.cin);
  WS_READY(h, ws, "workspace too small for mel");
  LAUNCH(h, s, "frame_pad", 0, 8.0 * B * rows * c.hop,
         dcx::launch_frame_pad(audio, fr.f, fr.p, B, n, rows, c.hop, (c.win - c.hop) / 2, s));
  ConvCall cc = framed(fr, B, rows, c.hop);
  cc.exact = true;
  cc.Lq = T;
  cc.y = spec;
  RUN(run_conv(h, h->dft, cc, s));
  return mel_from_spec(h, spec, mag, (long long)B * T, mel, loglin, s);
}

// stage_mel on a ragged batch: whole frames [sum T][n_fft] cut per clip (launch_ragged_frames), the DFT
// as a one-tap GEMM over them (dft1), then the row-wise tail.
static int stage_mel_ragged(dcx_codec* h, const float* audio, const dcx::RaggedSeg& rg, Act mel, Bump& ws, hipStream_t s) {
  const dcx_config& c = h->cfg;
  const long long M = rg.rows;
  Act fr = conv_input(h, ws, (size_t)M * c.n_fft);
  float* spec = ws.f((size_t)M * h->dft.cout);
  Act mag = conv_input(h, ws, (size_t)M * h->melfb.cin);
  WS_READY(h, ws, "workspace too small for mel");
  LAUNCH(h, s, "ragged_frames", 0, 10.0 * M * c.n_fft,
         dcx::launch_ragged_frames(audio, rg, fr.f, fr.p, c.n_fft, c.hop, (c.win - c.hop) / 2, s));
  ConvCall cc = pointwise(fr, M);
  cc.exact = true;
  cc.fixed_tiles = true;
  cc.y = spec;
  RUN(run_conv(h, h->dft1, cc, s));
  return mel_from_spec(h, spec, mag, M, mel, nullptr, s);
}

// Whether a call may fork its half-batches onto the side stream: a handle with one, not inside a
// half already (fork: the caller's word on that), not in the split-K latency mode (both halves would
// write their partial sums to the one h->split_buf at the same time, and a half's tile counts, so its
// slice counts and low bits, are not the whole batch's), and a caller's stream that is not being
// captured into a hipGraph (a captured call keeps to the caller's stream, with the same bits)
static bool may_fork(dcx_codec* h, hipStream_t s, bool fork) {
  if (!h->side || !fork || h->split_k >= 2) return false;
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  return hipStreamIsCapturing(s, &st) == hipSuccess && st == hipStreamCaptureStatusNone;
}

// first() on the caller's stream s and second() on the side stream, which is forked from and joined to
// s by events; second() is skipped when first() fails.
template <class F0, class F1>
static int fork_join(dcx_codec* h, hipStream_t s, F0 first, F1 second) {
  HIPCHK(h, hipEventRecord(h->fork_ev, s));
  HIPCHK(h, hipStreamWaitEvent(h->side, h->fork_ev, 0));
  const int rc0 = first();
  const int rc1 = rc0 != DCX_OK ? rc0 : second();
  // joined whatever happened, so the caller's stream never runs ahead of the side stream's work
  const hipError_t e0 = hipEventRecord(h->join_ev, h->side);
  const hipError_t e1 = hipStreamWaitEvent(s, h->join_ev, 0);
  RUN(rc1);
  HIPCHK(h, e0);
  HIPCHK(h, e1);
  return DCX_OK;
}

// Rows [r0, ...) (clips b0 on) of a [B][T][C] activation in its layout, with its per-row and per-clip
// range pointers.
// The three a.r offsets are unreached today, so no test exercises them: the activations that are split
// carry no consumer-side ranges (mel has none, feat's consumer reads the whole batch's table through
// the unsplit Act, z carries none).  The live offsets of a split are the producer-side row_ash /
// row_amax in act_rows_out and scratch_rows.
template <class A>
static A act_rows(A a, int b0, long long r0, long long C) {
  if (a.f) a.f += r0 * C;
  if (a.p) a.p += r0 * C * layout_u16(a.lay);
  if (a.r.ash) a.r.ash += b0;
  if (a.r.amax) a.r.amax += b0;
  if (a.r.ash_row) a.r.ash_row += r0;
  return a;
}
static Act act_rows_out(Act a, int b0, long long r0, long long C) {
  a = act_rows(a, b0, r0, C);
  if (a.row_ash) a.row_ash += r0;
  if (a.row_amax) a.row_amax += r0;
  return a;
}
// A conv-input scratch region (conv_input: planes-sized) of n elements per row, from row r0 on.
static Act scratch_rows(Act a, long long r0, long long n) {
  if (a.f) a.f += r0 * n;
  if (a.p) a.p += r0 * n * 3;
  if (a.row_ash) a.row_ash += r0;
  if (a.row_amax) a.row_amax += r0;
  return a;
}

// The encoder (encoders.py:68-76) on clips of one batch: stem conv + LN, 4 stages of (LN +
// downsample 1x1 conv) and ConvNeXt blocks, the final LayerNorm into feat.
// rg: a ragged batch (B = 1, T = its total frames).  The stem then reads the mel rows unfolded per
// clip into the hidden scratch (free until the first block) as a one-tap GEMM (stem1), and every
// block's depthwise conv stays inside its clip.
static int encode_clips(dcx_codec* h, const CAct& mel, int B, int T, Act feat, float* xa, float* xb, Act ln, Act hid,
                 hipStream_t s, const dcx::RaggedSeg* rg = nullptr) {
  const dcx_config& c = h->cfg;
  const long long M = (long long)B * T;
  if (rg) {
    if (!mel.p || !hid.p || mel.lay != LAYOUT_PLANES) return fail(h, DCX_ERR_STATE, "internal: ragged stem needs planes");
    LAUNCH(h, s, "ragged_unfold", 0, 6.0 * M * c.n_mels * (1 + h->stem.taps),
           dcx::launch_ragged_unfold(mel.p, hid.p, *rg, c.n_mels * 6, h->stem.taps, s));
    ConvCall cc = pointwise(CAct(nullptr, hid.p), M);
    cc.fixed_tiles = true;
    cc.y = xa;
    RUN(run_conv(h, h->stem1, cc, s));
  } else {
    ConvCall cc = framed(mel, B, T, c.n_mels);
    cc.y = xa;
    RUN(run_conv(h, h->stem, cc, s));
  }
  RUN(run_ln(h, h->stem_ln, xa, Act{xb, nullptr}, M, s, /*bf16_in=*/true));
  for (int i = 0; i < 4; ++i) {
    if (i > 0) {
      ln.lay = input_layout(h, h->ds_conv[i], M, ln.row_ash);  // h2: the downsample 1x1 conv on conv_gemm_x3dw
      ln.r = Rng{};
      ln.r.ash_row = ln.lay == LAYOUT_H2 ? ln.row_ash : nullptr;  // row-scaled by run_ln
      RUN(run_ln(h, h->ds_ln[i], xb, ln, M, s));
      ConvCall cd = pointwise(ln, M);
      cd.y = xb;
      RUN(run_conv(h, h->ds_conv[i], cd, s));
    }
    for (auto& bw : h->blocks[i]) RUN(run_block(h, bw, xb, nullptr, B, T, ln, hid, s, LAYOUT_PLANES, rg));
  }
  RUN(run_ln(h, h->enc_norm, xb, feat, M, s));  // an h2 feat: row-scaled into feat.row_ash
  return DCX_OK;
}

// Two half-batches on two streams (round 6, Knobs::enc_streams): the encoder's launches are short
// (the 1x1 convs of a C2 batch are 0.5-7 rounds of tiles over the CUs, e.g. pwconv2 at C = 768:
// 354 tiles = 1.38 rounds), so one half's partly filled last round runs beside the other half's
// launches.  Every kernel computes a clip's rows alone (tiles never span clips; per-row range
// scales), so the halves give the bits of the whole batch.  Not in the split-K latency mode, where
// neither holds (may_fork): the batch then runs on the caller's stream.
int stage_encode(dcx_codec* h, CAct mel, int B, int T, Act feat, Bump& ws, hipStream_t s, const dcx::RaggedSeg* rg,
                 bool fork) {
  const dcx_config& c = h->cfg;
  const long long M = (long long)B * T;
  const int cmax = c.enc_dims[3];
  RUN(ensure_planes(h, mel, M, c.n_mels, ws, s));
  float* xa = ws.f((size_t)M * cmax);
  float* xb = ws.f((size_t)M * cmax);
  Act ln = conv_input(h, ws, (size_t)M * cmax);
  Act hid = conv_input(h, ws, (size_t)M * 4 * cmax);
  row_ranges(h, ws, M, ln, hid);
  WS_READY(h, ws, "workspace too small for encode");
  if (rg || B < 2 || !h->knobs.enc_streams || !may_fork(h, s, fork))
    return encode_clips(h, mel, B, T, feat, xa, xb, ln, hid, s, rg);
  const int B0 = (B + 1) / 2;
  const long long r1 = (long long)B0 * T;
  return fork_join(
      h, s, [&] { return encode_clips(h, mel, B0, T, feat, xa, xb, ln, hid, s); },
      [&] {
        return encode_clips(h, act_rows(mel, B0, r1, c.n_mels), B - B0, T, act_rows_out(feat, B0, r1, cmax),
                            xa + r1 * cmax, xb + r1 * cmax, scratch_rows(ln, r1, cmax),
                            scratch_rows(hid, r1, 4LL * cmax), h->side);
      });
}

// x_pjt_in layout the nearest-code search reads: compact bf16 for vq_prefilter_b1 (x6 and bf16
// modes), else planes (vq_prefilter_dm / _x3; fp32 mode ignores it).
Layout vq_xlayout(const dcx_codec* h) { return x6_mode(h) && h->compact && h->vq[0].codebook_b1 ? LAYOUT_BF16 : LAYOUT_PLANES; }

// The nearest-code search of DownsampleGRVQ (vector_quantize_pytorch.py:41-45, 496-506; first index on
// ties) on x_pjt_in P (fp32 [M][CD]) and, in x6 / bf16 mode, P6 in the prefilter's layout xl (planes or
// compact bf16): |x|^2, the certified prefilter and the fp64 rescore (x6 / bf16), or the exact
// fp32 distance GEMM and its reduce (fp32 mode).  pv / pi / pv2: [M][ntiles] scratch, x2: [M].
// Workspace of one search of M rows: the prefilter's [M][ntiles] partials and, in x6 / bf16 mode, the
// rescore's candidate list (128 pairs per row on average: the C2 workload lists 62 in x6 mode; a row that does not fit is rescored in place).
VqScratch vq_scratch(const dcx_codec* h, Bump& ws, long long M, int ntiles, bool x6) {
  VqScratch v;
  v.x2 = ws.f((size_t)M);
  v.pv = ws.f((size_t)M * ntiles);
  v.pi = ws.i((size_t)M * ntiles);
  if (x6) {
    v.xr2 = ws.f((size_t)M);
    v.pv2 = ws.f((size_t)M * ntiles);
    v.x2d = (double*)ws.raw((size_t)M * sizeof(double));
    // list offsets are stored as int (row_list): at most INT_MAX pairs; rows beyond are rescored in place
    v.cap = h->vq_pairs_per_row > 0
                ? std::min<long long>(std::max<long long>((long long)h->vq_pairs_per_row * M, 1024), INT_MAX) / 8 * 8
                : 0;
    v.pairs = (int2*)ws.raw((size_t)v.cap * sizeof(int2));
    v.cdist = (double*)ws.raw((size_t)(v.cap / 8) * sizeof(double));
    v.ccode = ws.i((size_t)(v.cap / 8));
    v.row_list = (int2*)ws.raw((size_t)M * sizeof(int2));
    v.npairs = (unsigned long long*)ws.raw(sizeof(unsigned long long));
  }
  return v;
}

int run_vq_search(dcx_codec* h, int layer, const float* P, const unsigned short* P6, Layout xl, long long M,
                  const VqScratch& v, int ntiles, int32_t* codes, hipStream_t s, bool x_bf16, bool have_norms) {
  const dcx_config& c = h->cfg;
  const dcx_codec::VqLayer& L = h->vq[layer];
  const int CD = c.codebook_dim, NC = c.codebook_size;
  const bool x6 = x6_mode(h);
  const bool b1 = xl == LAYOUT_BF16 && dcx::vq_b1_takes(NC, CD);
  float* const x2 = v.x2;
  if (!have_norms)
    LAUNCH(h, s, "row_sqnorm", 2.0 * M * CD, 4.0 * M * CD,
           dcx::launch_row_sqnorm(P, M, CD, x2, x6 ? v.x2d : nullptr, b1 ? v.xr2 : nullptr, x6 ? v.npairs : nullptr, s));
  {
    ConvParams p{};
    p.x = P; p.x6 = P6; p.w = L.codebook; p.w6 = x6 ? L.codebook6 : nullptr;
    p.Cin = CD; p.Cout = NC; p.ldx = CD; p.taps = 1; p.in_step = 1; p.out_mul = 1;
    p.x2 = x2; p.e2 = L.e2; p.part_val = v.pv; p.part_idx = v.pi; p.part_val2 = v.pv2;
    p.x_layout = xl;
    p.wc = b1 ? L.codebook_b1 : nullptr;
    ProfScope ps(h, s);
    const char* kname = "vq";
    if (x6) {
      // x_bf16: bf16 mode rounds x_pjt_in to bf16 in the project_in epilogue (round_bf16); a later
      // layer's residual is not bf16-valued and takes the general form
      HIPCHK(h, dcx::launch_vq_prefilter(p, (int)M, x_bf16, s, &kname));
      ps.done(kname, 2.0 * M * NC * CD, 4.0 * ((double)M * CD + (double)NC * CD));
    } else {
      HIPCHK(h, dcx::launch_vq_argmin(p, (int)M, s, &kname));
      ps.done(kname, 2.0 * M * NC * CD, 4.0 * ((double)M * CD + (double)NC * CD));
    }
  }
  if (x6) {
    dcx::VqRescoreArgs a{};
    a.part_val = v.pv; a.part_val2 = v.pv2; a.part_idx = v.pi;
    a.rows = M; a.ntiles = ntiles; a.tile_codes = NC / ntiles; a.dim = CD;
    a.x = P; a.x2 = x2; a.xr2 = b1 ? v.xr2 : nullptr; a.x2d = v.x2d;
    a.codebook = L.codebook; a.e2d = L.e2d;
    a.cx = dcx::vq_prefilter_cx(xl, NC, CD, L.emax, L.dmax); a.emax = L.emax; a.e2max = L.e2max;
    a.codes = codes; a.stats = h->vq_stats_on ? h->vq_stats : nullptr;
    a.pairs = v.pairs; a.cdist = v.cdist; a.ccode = v.ccode; a.cap = v.cap; a.row_list = v.row_list; a.npairs = v.npairs;
    LAUNCH(h, s, "vq_certify", 0, 12.0 * M * ntiles + 4.0 * M, dcx::launch_vq_certify(a, s));
    LAUNCH(h, s, "vq_pair_eval", 0, 0, dcx::launch_vq_pair_eval(a, s));
    LAUNCH(h, s, "vq_pair_reduce", 0, 0, dcx::launch_vq_pair_reduce(a, s));
  } else {
    LAUNCH(h, s, "vq_reduce", 0, 8.0 * M * ntiles, dcx::launch_vq_reduce(v.pv, v.pi, (int)M, ntiles, codes, s));
  }
  return DCX_OK;
}

// decode table in planes for this mode's gathers: project_out in fp32 (x6) or under autocast (bf16)
static const unsigned short* decode_table6(const dcx_codec* h) {
  return h->gemm_mode == DCX_GEMM_BF16 && h->ptable6b ? h->ptable6b : h->ptable6;
}

// The decode-table rows of M codes into zd (a conv_input: planes in x6 / bf16 mode, else fp32);
// n_invalid: optional count of codes outside the codebook (they take the masked code's row)
// lens / T (ragged batches): the rows are clips of T codes, those at or beyond lens[clip] are not read
// A chain (R > 1; codes [M][R]) decodes in the reference's order (residual_vq.py:103-138): the layers'
// rows summed in fp32 into qs (project_out's input: fp32, or planes / compact bf16, whose hi plane is
// bf16(sum) for the bf16 mode's autocast), then project_out as a 1x1 conv into zd in vq_up's layout.
static int gather_decoded(dcx_codec* h, const int32_t* codes, long long M, Act zd, Act qs, int32_t* n_invalid,
                          hipStream_t s, const int* lens = nullptr, int T = 0) {
  const int D = h->cfg.vq_dim, NC = h->cfg.codebook_size, R = h->n_layers;
  if (R > 1) {
    const int CD = h->cfg.codebook_dim;
    dcx::GatherSumArgs g{};
    for (int k = 0; k < R; ++k) g.table[k] = h->vq[k].codebook;
    g.idx = codes; g.out = qs.f; g.out6 = qs.p; g.out_layout = qs.lay; g.n_invalid = n_invalid;
    g.clip_len = lens; g.frames = T; g.rows = M; g.dim = CD; g.ncodes = NC; g.R = R;
    LAUNCH(h, s, "gather_sum_rows", 1.0 * M * CD * (R - 1), 4.0 * M * CD * R + (qs.p ? 2.0 * layout_u16(qs.lay) : 4.0) * M * CD,
           dcx::launch_gather_sum_rows(g, s));
    ConvCall co = pointwise(qs, M);
    co.out_to(zd);
    return run_conv(h, h->vq_pout, co, s);
  }
  if (x6_mode(h))
    LAUNCH(h, s, "gather_rows", 0, 12.0 * M * D,
           dcx::launch_gather_rows((const float*)decode_table6(h), NC, codes, M, D * 3 / 2, (float*)zd.p, n_invalid, NC, s,
                                   lens, T));
  else
    LAUNCH(h, s, "gather_rows", 0, 8.0 * M * D,
           dcx::launch_gather_rows(h->ptable, NC, codes, M, D, zd.f, n_invalid, NC, s, lens, T));
  return DCX_OK;
}

// project_out's input of a chain's decode: M rows of codebook_dim in the layout the conv reads in this
// mode (fp32; compact bf16 where conv_gemm_bf16dm takes it; else planes).  Nothing for one codebook.
static Act alloc_qsum(dcx_codec* h, Bump& ws, long long M) {
  Act qs;
  if (h->n_layers < 2) return qs;
  const size_t n = (size_t)M * h->cfg.codebook_dim;
  if (!x6_mode(h)) {
    qs.f = ws.f(n);
    return qs;
  }
  qs.lay = takes_compact(h, h->vq_pout, M) ? LAYOUT_BF16 : LAYOUT_PLANES;
  qs.p = ws.u16(n * 3);  // planes-sized in either layout, as conv_input: the size does not follow the mode's kernels
  return qs;
}

int stage_vq_encode(dcx_codec* h, CAct feat, int B, int T, int32_t* codes, float* pin, float* fup, float* quant,
                    Bump& ws, hipStream_t s, const dcx::RaggedSeg* rg) {
  const dcx_config& c = h->cfg;
  const long long M = (long long)B * T;
  const int D = c.vq_dim, CD = c.codebook_dim, NC = c.codebook_size;
  const bool x6 = x6_mode(h);
  const Layout xl = vq_xlayout(h);
  const int ntiles = x6 ? dcx::vq_prefilter_ntiles(NC, CD, xl) : dcx::vq_argmin_ntiles(NC);
  // the down conv's input as the fused pipeline writes it: compact bf16 (bf16 mode) or h2 (h3), the
  // latter scaled per row by the row's exact max as the encoder's final LayerNorm scales it, so the
  // staged and the fused call compute the same bits
  RUN(ensure_planes(h, feat, M, D, ws, s, input_layout(h, h->vq_down, M), 0));
  if (feat.lay == LAYOUT_BF16 && !takes_compact(h, h->vq_down, M)) return fail(h, DCX_ERR_STATE, "internal: compact features");
  float* X = ws.f((size_t)M * D);
  unsigned short* X6 = x6 ? ws.u16((size_t)M * D * 3) : nullptr;
  Act ln = conv_input(h, ws, (size_t)M * D);
  Act hid = conv_input(h, ws, (size_t)M * 4 * D);
  row_ranges(h, ws, M, ln, hid);
  int* x6_ash = x6 ? ws.i((size_t)M) : nullptr;  // project_in's input rows' shifts (h3)
  float* P = pin ? pin : ws.f((size_t)M * CD);
  unsigned short* P6 = x6 ? ws.u16((size_t)M * CD * 3) : nullptr;
  const VqScratch vs = vq_scratch(h, ws, M, ntiles, x6);
  Act zd = conv_input(h, ws, (size_t)M * D);
  // a chain: the fp32 residual (x_pjt_in itself is kept: the caller may have asked for it), one layer's
  // codes as the search writes them, and project_out's input
  const int R = h->n_layers;
  float* Rs = R > 1 ? ws.f((size_t)M * CD) : nullptr;
  int32_t* ck = R > 1 ? ws.i((size_t)M) : nullptr;
  Act qs = alloc_qsum(h, ws, M);
  WS_READY(h, ws, "workspace too small for vq_encode");
  ConvCall cd = pointwise(feat, M);
  cd.y = X;
  RUN(run_conv(h, h->vq_down, cd, s));
  const Layout xp = X6 ? input_layout(h, h->vq_pin, M) : LAYOUT_PLANES;
  const bool h2p = xp == LAYOUT_H2;  // project_in on conv_gemm_x3dw
  // the block's output for project_in: compact / planes from its epilogue, or (h3) split per row by
  // the row's exact max afterwards (launch_h2_rows)
  RUN(run_block(h, h->vq_down_blk, X, h2p ? nullptr : X6, B, T, ln, hid, s, xp, rg));
  if (h2p) LAUNCH(h, s, "h2_rows", 0, 8.0 * M * D, dcx::launch_h2_rows(X, X6, M, D, x6_ash, s));
  CAct pin_in(X, X6, xp);
  if (h2p) pin_in.r.ash_row = x6_ash;
  ConvCall cp = pointwise(pin_in, M);
  cp.y = P;
  cp.y6 = P6;
  cp.y_lay = xl;
  RUN(run_conv(h, h->vq_pin, cp, s));
  const bool bf16 = h->gemm_mode == DCX_GEMM_BF16;
  if (R == 1) {
    RUN(run_vq_search(h, 0, P, P6, xl, M, vs, ntiles, codes, s, bf16));
    if (fup) LAUNCH(h, s, "gather_rows", 0, 8.0 * M * CD, dcx::launch_gather_rows(h->vq[0].codebook, NC, codes, M, CD, fup, nullptr, -1, s));
  }
  // the chain (residual_vq.py:208-259): layer k searches r_k, then one pass writes its codes into
  // column k, adds its rows to fup and leaves r_{k+1} = fl32(r_k - E_k[c_k]) with everything the next
  // search reads (its operand image, its row norms, the zeroed pair counter)
  for (int k = 0; R > 1 && k < R; ++k) {
    RUN(run_vq_search(h, k, k ? Rs : P, P6, xl, M, vs, ntiles, ck, s, bf16 && k == 0, /*have_norms=*/k > 0));
    const bool last = k == R - 1;
    const bool b1 = xl == LAYOUT_BF16 && dcx::vq_b1_takes(NC, CD);
    dcx::VqResidualArgs a{};
    a.src = k ? Rs : P; a.codebook = h->vq[k].codebook; a.ck = ck; a.codes_out = codes + k;
    a.dst = last ? nullptr : Rs; a.op6 = last ? nullptr : P6; a.op_layout = xl;
    a.x2 = last ? nullptr : vs.x2; a.x2d = last || !x6 ? nullptr : vs.x2d; a.xr2 = last || !b1 ? nullptr : vs.xr2;
    a.zero_me = last || !x6 ? nullptr : vs.npairs;
    a.fup = fup; a.fup_first = k == 0; a.rows = M; a.dim = CD; a.ncodes = NC; a.R = R;
    const double rw = (last ? 0.0 : 8.0 + (P6 ? 2.0 * layout_u16(xl) : 0.0)) + (fup ? (k ? 8.0 : 4.0) : 0.0);
    LAUNCH(h, s, "vq_residual_step", last ? 0.0 : 3.0 * M * CD, (4.0 + rw) * M * CD, dcx::launch_vq_residual_step(a, s));
  }
  if (quant) {
    RUN(gather_decoded(h, codes, M, zd, qs, nullptr, s));
    ConvCall cu = pointwise(zd, M);
    cu.y = quant;
    RUN(run_conv(h, h->vq_up, cu, s));
    RUN(run_block(h, h->vq_up_blk, quant, nullptr, B, T, ln, hid, s, LAYOUT_PLANES, rg));
  }
  return DCX_OK;
}

// z.f is required (fp32 residual stream of the up-path block); z.p optionally receives planes.
int stage_vq_decode(dcx_codec* h, const int32_t* codes, int B, int T, Act z, int32_t* n_invalid, Bump& ws,
                    hipStream_t s, const int* lens) {
  const dcx_config& c = h->cfg;
  const long long M = (long long)B * T;
  const int D = c.vq_dim;
  Act zd = conv_input(h, ws, (size_t)M * D);
  Act ln = conv_input(h, ws, (size_t)M * D);
  Act hid = conv_input(h, ws, (size_t)M * 4 * D);
  row_ranges(h, ws, M, ln, hid);
  Act qs = alloc_qsum(h, ws, M);
  WS_READY(h, ws, "workspace too small for vq_decode");
  if (z.p && z.lay == LAYOUT_H2) return fail(h, DCX_ERR_STATE, "internal: z in h2 is split by the generator (ranged per clip)");
  RUN(gather_decoded(h, codes, M, zd, qs, n_invalid, s, lens, T));
  ConvCall cu = pointwise(zd, M);
  cu.y = z.f;
  RUN(run_conv(h, h->vq_up, cu, s));
  // ragged batches: the block's depthwise conv is the one step here that reads neighbouring rows; with
  // its input zero from each clip's length on it sees the padding the clip has alone.  The block's
  // rows beyond the lengths are computed and never read (the generator bounds z by the same lengths).
  if (lens)
    LAUNCH(h, s, "zero_tail_rows", 0, 0, dcx::launch_zero_tail_rows(z.f, B, T, D, lens, 1, s));
  RUN(run_block(h, h->vq_up_blk, z.f, z.p, B, T, ln, hid, s));
  return DCX_OK;
}

// conv_pre's input z of B clips x T frames: fp32, plus planes from the VQ up block's epilogue (x6)
// unless the generator splits z.f into h2 itself with each clip's exact range (launch_h2_ranged)
static Act alloc_z(dcx_codec* h, Bump& ws, int B, int T) {
  const long long M = (long long)B * T;
  Act z;
  z.f = ws.f((size_t)M * h->cfg.vq_dim);
  if (x6_mode(h) && !(h->has_gen && takes_h3_conv(h, h->conv_pre, T))) z.p = ws.u16((size_t)M * h->cfg.vq_dim * 3);
  return z;
}

// mel -> encoder -> VQ encode -> VQ decode of B clips, into z (the generator's input)
// fork: whether the encoder may put its second half-batch on the side stream (not inside a half)
static int encode_clips_to_z(dcx_codec* h, const float* audio, int B, int64_t n, int32_t* codes, Act z, Bump& ws,
                             hipStream_t s, bool fork) {
  const dcx_config& c = h->cfg;
  const int T = (int)frames_of(c, n);
  const long long M = (long long)B * T;
  Act mel = conv_input(h, ws, (size_t)M * c.n_mels);
  Act feat = conv_input(h, ws, (size_t)M * c.enc_dims[3]);
  // written by the encoder's final LayerNorm: compact (bf16 mode), or h2 for the quantizer's down conv (x3dw)
  feat.lay = input_layout(h, h->vq_down, M);
  // (reserved whenever x6 mode could write it: a dry run sees no pointers, so sizes must not depend on them)
  if (x6_mode(h)) feat.row_ash = ws.i((size_t)M);
  if (feat.lay == LAYOUT_H2) feat.r.ash_row = feat.row_ash;  // scaled per row by the final LayerNorm (its exact row maxima)
  const size_t mark = ws.off;
  size_t need = mark;
  auto sub = [&](auto fn) -> int {  // each sub-stage reuses the tail of the workspace
    Bump tail(ws.base, ws.cap, ws.dry);
    tail.off = mark;
    int rc = fn(tail);
    need = std::max(need, tail.off);
    return rc;
  };
  if (!ws.dry && !ws.ok()) return fail(h, DCX_ERR_WORKSPACE, "workspace too small for encode_decode");
  RUN(sub([&](Bump& t) { return stage_mel(h, audio, B, n, mel, t, s); }));
  RUN(sub([&](Bump& t) { return stage_encode(h, CAct(mel), B, T, feat, t, s, nullptr, fork); }));
  RUN(sub([&](Bump& t) { return stage_vq_encode(h, CAct(feat), B, T, codes, nullptr, nullptr, nullptr, t, s); }));
  RUN(sub([&](Bump& t) { return stage_vq_decode(h, codes, B, T, z, nullptr, t, s); }));
  ws.off = need;
  return DCX_OK;
}

// packed audio -> packed mel -> encoder -> VQ search on the rows of a ragged batch: the stages of
// encode_clips_to_z on one "clip" of rg.rows rows, the three clip-aware steps segment-aware
int tokenize_ragged_rows(dcx_codec* h, const float* audio, const dcx::RaggedSeg& rg, int32_t* codes, float* pin,
                         float* fup, Bump& ws, hipStream_t s) {
  const dcx_config& c = h->cfg;
  const long long M = rg.rows;
  Act mel = conv_input(h, ws, (size_t)M * c.n_mels);
  Act feat = conv_input(h, ws, (size_t)M * c.enc_dims[3]);
  feat.lay = input_layout(h, h->vq_down, M);
  if (x6_mode(h)) feat.row_ash = ws.i((size_t)M);
  if (feat.lay == LAYOUT_H2) feat.r.ash_row = feat.row_ash;
  const size_t mark = ws.off;
  size_t need = mark;
  auto sub = [&](auto fn) -> int {  // each sub-stage reuses the tail of the workspace
    Bump tail(ws.base, ws.cap, ws.dry);
    tail.off = mark;
    int rc = fn(tail);
    need = std::max(need, tail.off);
    return rc;
  };
  if (!ws.dry && !ws.ok()) return fail(h, DCX_ERR_WORKSPACE, "workspace too small for tokenize_ragged");
  RUN(sub([&](Bump& t) { return stage_mel_ragged(h, audio, rg, mel, t, s); }));
  RUN(sub([&](Bump& t) { return stage_encode(h, CAct(mel), 1, (int)M, feat, t, s, &rg); }));
  RUN(sub([&](Bump& t) { return stage_vq_encode(h, CAct(feat), 1, (int)M, codes, pin, fup, nullptr, t, s, &rg); }));
  ws.off = need;
  return DCX_OK;
}

// a finalized handle without generator weights can never run the generator: its size is left out
// of the workspace (token extraction at C3's 256 clips would otherwise reserve 139 GB)
static bool sizes_generator(const dcx_codec* h, const Bump& ws) { return !(ws.dry && h->finalized && !h->has_gen); }

static int encode_decode_clips(dcx_codec* h, const float* audio, int B, int64_t n, int32_t* codes, float* wav, Bump& ws,
                               hipStream_t s, bool fork) {
  const int T = (int)frames_of(h->cfg, n);
  Act z = alloc_z(h, ws, B, T);
  const size_t mark = ws.off;
  Bump front(ws.base, ws.cap, ws.dry);
  front.off = mark;
  RUN(encode_clips_to_z(h, audio, B, n, codes, z, front, s, fork));
  size_t need = front.off;
  if (sizes_generator(h, ws)) {
    Bump tail(ws.base, ws.cap, ws.dry);
    tail.off = mark;
    RUN(stage_generate(h, CAct(z), B, T, wav, tail, s));
    need = std::max(need, tail.off);
  }
  if (ws.dry) ws.off = need;
  return DCX_OK;
}

// codes -> z -> waveform of a ragged batch in the padded layout (dcx_decode_ragged): z and the VQ
// decode's scratch are a part of what encode_decode_clips carves for the same (B, T), so
// dcx_workspace_size covers the call.  One stream: no half-batch fork.
int stage_decode_ragged(dcx_codec* h, const int32_t* codes, const int* lens, int B, int T, float* wav,
                        int32_t* n_invalid, Bump& ws, hipStream_t s) {
  Act z;
  z.f = ws.f((size_t)B * T * h->cfg.vq_dim);  // fp32 alone: the generator splits it per clip (stage_generate checks)
  const size_t mark = ws.off;
  Bump front(ws.base, ws.cap, ws.dry);
  front.off = mark;
  RUN(stage_vq_decode(h, codes, B, T, z, n_invalid, front, s, lens));
  Bump tail(ws.base, ws.cap, ws.dry);
  tail.off = mark;
  return stage_generate(h, CAct(z), B, T, wav, tail, s, lens);
}

// One step of a token stream (dcx_stream_decode_step): the slots' plan, their windows of codes, the
// ragged decode of the windows as dcx_decode_ragged runs it for (sessions, W), and the emitted frames.
// The emit kernel commits the slots' counters, so a step that fails before it leaves the state as it was.
int stage_stream_step(dcx_codec* h, const dcx::StreamState& st, const int32_t* new_codes, const int* n_new,
                      const int* flags, float* wav_out, int* n_out, int32_t* n_invalid, Bump& ws, hipStream_t s) {
  const double codes = (double)st.sessions * st.W * st.R;
  LAUNCH(h, s, "stream_plan", 0, 4.0 * dcx::kStreamCounters * st.sessions, dcx::launch_stream_plan(st, n_new, flags, s));
  LAUNCH(h, s, "stream_window", 0, 8.0 * codes, dcx::launch_stream_window(st, new_codes, h->cfg.codebook_size, n_invalid, s));
  // the appended codes were counted once, as they arrived: the decode would count a bad code again in
  // every window that holds it
  RUN(stage_decode_ragged(h, st.window, st.len, st.sessions, st.W, st.wav, nullptr, ws, s));
  LAUNCH(h, s, "stream_emit", 0, 8.0 * st.sessions * (st.push + st.halo) * st.hop,
         dcx::launch_stream_emit(st, wav_out, n_out, s));
  return DCX_OK;
}

// dcx_tokenize_slots: tokenize_ragged_rows on the slot form of rg (every row of the padded layout, the
// three clip-aware steps bounded by the slots' device-side lengths), then the results beyond each
// slot's length set to -1 / zero.
int tokenize_slots_rows(dcx_codec* h, const float* audio, const dcx::RaggedSeg& rg, int32_t* codes, float* pin, Bump& ws,
                        hipStream_t s) {
  RUN(tokenize_ragged_rows(h, audio, rg, codes, pin, nullptr, ws, s));
  if (ws.dry) return DCX_OK;
  LAUNCH(h, s, "slots_mask", 0, 0, dcx::launch_slots_mask(rg, codes, h->n_layers, pin, h->cfg.codebook_dim, s));
  return DCX_OK;
}

// One step of an audio stream (dcx_stream_encode_step): the slots' plan, their windows of samples, the
// slot tokenization of the windows with the plan's lengths, and the emitted codes.  The emit kernel
// commits the slots' counters, so a step that fails before it leaves the state as it was.
int stage_audio_stream_step(dcx_codec* h, const dcx::AudioStreamState& st, const dcx::RaggedSeg& rg,
                            const float* new_samples, const int* n_new, const int* flags, int32_t* codes_out, int* n_out,
                            float* pin_out, Bump& ws, hipStream_t s) {
  const double samples = (double)st.sessions * st.Ws;
  LAUNCH(h, s, "audio_stream_plan", 0, 4.0 * dcx::kAudioStreamCounters * st.sessions,
         dcx::launch_audio_stream_plan(st, n_new, flags, s));
  LAUNCH(h, s, "audio_stream_window", 0, 8.0 * samples, dcx::launch_audio_stream_window(st, new_samples, s));
  RUN(tokenize_slots_rows(h, st.window, rg, st.codes, st.pin, ws, s));
  LAUNCH(h, s, "audio_stream_emit", 0, 8.0 * st.sessions * st.K * (st.R + (pin_out ? st.CD : 0)),
         dcx::launch_audio_stream_emit(st, codes_out, n_out, pin_out, s));
  return DCX_OK;
}

// Half-batches on two streams (Knobs::enc_streams >= 2; 1 forks inside the encoder only): clips
// [0, B0) on the caller's stream and [B0, B) on the side stream, each in its own part of the
// workspace (half 0's, then half 1's: the sizes are linear in the clip count).  Every stage computes
// a clip alone (the reference's batch semantics: clips padded to one length, no cross-clip
// arithmetic), so the halves give the bits of the whole batch; the encoder then runs unforked inside
// each half.  2 (default): mel -> encoder -> VQ encode -> VQ decode per half, joined, then the
// generator on the whole batch, so the generator's long launches (the dominant kernel) run alone;
// 3: the generator per half too.  Not in the split-K latency mode, whose partial sums share one
// scratch region: no level forks there (may_fork refuses, so the encoder inside the one-stream plan
// below stays on the caller's stream too), and the workspace is sized for that plan alone (the
// test on split_k here: a dry run does not ask may_fork).
int stage_encode_decode(dcx_codec* h, const float* audio, int B, int64_t n, int32_t* codes, float* wav, Bump& ws,
                        hipStream_t s) {
  const int mode = h->knobs.enc_streams;
  if (B < 2 || mode < 2 || h->split_k >= 2 || (!ws.dry && !may_fork(h, s, true)))
    return encode_decode_clips(h, audio, B, n, codes, wav, ws, s, /*fork=*/true);
  const int B0 = (B + 1) / 2;
  const int T = (int)frames_of(h->cfg, n);
  const size_t start = ws.off;
  Act z;
  if (mode == 2) z = alloc_z(h, ws, B, T);
  const size_t mark = ws.off;
  // the halves' parts: [mark, e0) and [e0, e1) (sized by dry runs)
  auto half = [&](int b0, int nb, Bump& w, hipStream_t st) -> int {
    const bool dry = w.dry;
    const float* a = dry ? nullptr : audio + (long long)b0 * n;
    int32_t* cd = dry ? nullptr : codes + (long long)b0 * T * h->n_layers;
    // inside a half the encoder does not fork again
    if (mode == 2)
      return encode_clips_to_z(h, a, nb, n, cd, act_rows_out(z, b0, (long long)b0 * T, h->cfg.vq_dim), w, st, /*fork=*/false);
    return encode_decode_clips(h, a, nb, n, cd, dry ? nullptr : wav + (long long)b0 * T * h->cfg.hop, w, st, /*fork=*/false);
  };
  Bump d0(nullptr, 0, true);
  d0.off = mark;
  RUN(half(0, B0, d0, s));
  Bump d1(nullptr, 0, true);
  d1.off = d0.off;
  RUN(half(B0, B - B0, d1, s));
  size_t need = d1.off;
  if (mode == 2 && sizes_generator(h, ws)) {
    Bump dg(nullptr, 0, true);
    dg.off = mark;
    RUN(stage_generate(h, CAct(z), B, T, nullptr, dg, s));
    need = std::max(need, dg.off);
  }
  if (ws.dry) {  // sized for the one-stream plan too (a call captured into a hipGraph does not fork)
    Bump one(nullptr, 0, true);
    one.off = start;
    RUN(encode_decode_clips(h, nullptr, B, n, nullptr, nullptr, one, s, /*fork=*/false));
    ws.off = std::max(need, one.off);
    return DCX_OK;
  }
  if (need > ws.cap) return fail(h, DCX_ERR_WORKSPACE, "workspace too small for encode_decode");
  Bump w0(ws.base, ws.cap, false), w1(ws.base, ws.cap, false);
  w0.off = mark;
  w1.off = d0.off;
  RUN(fork_join(h, s, [&] { return half(0, B0, w0, s); }, [&] { return half(B0, B - B0, w1, h->side); }));
  if (mode == 2) {
    Bump tail(ws.base, ws.cap, false);
    tail.off = mark;
    RUN(stage_generate(h, CAct(z), B, T, wav, tail, s));
  }
  return DCX_OK;
}

}  // namespace dcx::host
