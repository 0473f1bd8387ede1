// Single reference modules through the stages' launches (dcx_module_io, dcx_module_forward).
#include "dcx_host.h"

namespace dcx::host {

// "<prefix>.%d[.%d]" matched exactly (the whole name consumed).
static bool match_idx(const std::string& m, const char* fmt, int* a, int* b = nullptr) {
  int n = -1;
  const int want = b ? 2 : 1;
  const int got = b ? std::sscanf(m.c_str(), fmt, a, b, &n) : std::sscanf(m.c_str(), fmt, a, &n);
  return got == want && n == (int)m.size();
}

// Input / output widths of a module (dcx_module_io): cin, cout (0: int32 codes), output rows per
// input row.  False for unknown names.
bool module_io(const dcx_codec* h, const std::string& m, int& cin, int& cout, int& rate) {
  const dcx_config& c = h->cfg;
  int a = -1, b = -1;
  rate = 1;
  auto set = [&](int i, int o) {
    cin = i;
    cout = o;
    return true;
  };
  if (match_idx(m, "encoder.stages.%d.%d%n", &a, &b) && a >= 0 && a < 4 && b >= 0 && b < c.enc_depths[a])
    return set(c.enc_dims[a], c.enc_dims[a]);
  if (m == "encoder.downsample_layers.0") return set(c.n_mels, c.enc_dims[0]);
  if (m == "encoder.downsample_layers.0.1") return set(c.enc_dims[0], c.enc_dims[0]);
  if (match_idx(m, "encoder.downsample_layers.%d%n", &a) && a >= 1 && a < 4) return set(c.enc_dims[a - 1], c.enc_dims[a]);
  if (match_idx(m, "encoder.downsample_layers.%d.0%n", &a) && a >= 1 && a < 4) return set(c.enc_dims[a - 1], c.enc_dims[a - 1]);
  if (m == "encoder.norm") return set(c.enc_dims[3], c.enc_dims[3]);
  if (m == "quantizer.downsample.0" || m == "quantizer.downsample.0.1" || m == "quantizer.upsample.0" ||
      m == "quantizer.upsample.0.1")
    return set(c.vq_dim, c.vq_dim);
  if (m == "quantizer.grvq.rvqs.0.project_in") return set(c.vq_dim, c.codebook_dim);
  if (m == "quantizer.grvq.rvqs.0.project_out") return set(c.codebook_dim, c.vq_dim);
  if (m == "quantizer.search") return set(c.codebook_dim, 0);
  if (m == "generator.conv_pre") return set(c.vq_dim, c.gen_channels);
  int ch = c.gen_channels;
  for (int i = 0; i < c.n_ups; ++i) {
    if (m == "generator.ups." + std::to_string(i)) {
      rate = c.up_rates[i];
      return set(ch, ch / 2);
    }
    ch /= 2;
    if (match_idx(m, "generator.resblocks.%d.blocks.%d%n", &a, &b) && a == i && b >= 0 && b < c.n_res) return set(ch, ch);
    if (match_idx(m, "generator.resblocks.%d%n", &a) && a == i) return set(ch, ch);
  }
  if (m == "generator.conv_post") return set(ch, 1);
  return false;
}

// The input x [B][L][C] of a ResBlock as the generator's producers leave it: its per-clip max |.| in a
// slot of ra, and silu(x) in xs's form unless the convs apply it on load (silu_on_load), in h2
// range-scaled with its shift in a slot too.  xs.r becomes the range of x (and of silu(x)).
static int resblock_input(dcx_codec* h, const float* x, Act& xs, bool silu_on_load, int B, int L, int C,
                          RangeArena& ra, hipStream_t s) {
  const long long M = (long long)B * L;
  float* amax = ra.amax();
  xs.r = Rng{};
  xs.r.amax = amax;
  if (!silu_on_load && xs.lay == LAYOUT_H2) {
    int* sh = ra.ash();
    LAUNCH(h, s, "h2_ranged", 0, 12.0 * M * C,
           dcx::launch_h2_ranged(x, nullptr, xs.p, B, L, C, 1, 0.f, amax, sh, h->rflag, s));
    xs.r.ash = sh;
  } else {
    LAUNCH(h, s, "clip_amax", 0, 4.0 * M * C, dcx::launch_clip_amax(x, B, L, C, amax, s));
    if (!silu_on_load) LAUNCH(h, s, "silu_act", 0, 10.0 * M * C, dcx::launch_silu_act(x, xs.f, xs.p, M, C, s));
  }
  return DCX_OK;
}

// One module of the reference by its state-dict prefix, on the handle's packed weights and through
// the same launches the stages use.  x / y: channels-last fp32 [B][L][C] (codes int32 [B][L] for
// "quantizer.search").  See dcx_module_forward in the header for the list.
int stage_module(dcx_codec* h, const std::string& m, const float* x, int B, int L, void* yv, Bump& ws, hipStream_t s) {
  const dcx_config& c = h->cfg;
  const long long M = (long long)B * L;
  float* y = static_cast<float*>(yv);
  int a = -1, b = -1;
  // Sequential stems of the encoder (encoders.py:22-39): conv k7 + channels-first LayerNorm (i = 0),
  // LayerNorm + 1x1 conv (i >= 1)
  if (m == "encoder.downsample_layers.0") {
    CAct in(x, nullptr);
    RUN(ensure_planes(h, in, M, c.n_mels, ws, s));
    float* t = ws.f((size_t)M * c.enc_dims[0]);
    WS_READY(h, ws, "workspace too small for the module");
    ConvCall cc = framed(in, B, L, c.n_mels);
    cc.y = t;
    RUN(run_conv(h, h->stem, cc, s));
    return run_ln(h, h->stem_ln, t, Act{y, nullptr}, M, s, /*bf16_in=*/true);
  }
  if (match_idx(m, "encoder.downsample_layers.%d%n", &a) && a >= 1 && a < 4) {
    Act ln = conv_input(h, ws, (size_t)M * c.enc_dims[a - 1]);
    if (x6_mode(h)) ln.row_ash = ws.i((size_t)M);
    WS_READY(h, ws, "workspace too small for the module");
    ln.lay = input_layout(h, h->ds_conv[a], M, ln.row_ash);
    ln.r.ash_row = ln.lay == LAYOUT_H2 ? ln.row_ash : nullptr;
    RUN(run_ln(h, h->ds_ln[a], x, ln, M, s));
    ConvCall cd = pointwise(ln, M);
    cd.y = y;
    return run_conv(h, h->ds_conv[a], cd, s);
  }
  // the quantizer's down / up paths (grfvq.py:68-96): conv (k = factor) or ConvT, then a ConvNeXtBlock
  if (m == "quantizer.downsample.0" || m == "quantizer.upsample.0") {
    const bool down = m == "quantizer.downsample.0";
    const int D = c.vq_dim;
    CAct in(x, nullptr);
    // the down conv in h3 as in the pipeline (range floor: the encoder's final LayerNorm bound)
    RUN(ensure_planes(h, in, M, D, ws, s, h2_if(down && takes_h3(h, h->vq_down)), 0));
    Act ln = conv_input(h, ws, (size_t)M * D);
    Act hid = conv_input(h, ws, (size_t)M * 4 * D);
    row_ranges(h, ws, M, ln, hid);
    WS_READY(h, ws, "workspace too small for the module");
    ConvCall cc = pointwise(in, M);
    cc.y = y;
    RUN(run_conv(h, down ? h->vq_down : h->vq_up, cc, s));
    return run_block(h, down ? h->vq_down_blk : h->vq_up_blk, y, nullptr, B, L, ln, hid, s);
  }
  if (m == "quantizer.grvq.rvqs.0.project_in") {  // residual_vq.py:152
    CAct in(x, nullptr);
    RUN(ensure_planes(h, in, M, c.vq_dim, ws, s, h2_if(takes_h3(h, h->vq_pin)), 0));
    WS_READY(h, ws, "workspace too small for the module");
    ConvCall cp = pointwise(in, M);
    cp.y = y;
    return run_conv(h, h->vq_pin, cp, s);
  }
  if (m == "quantizer.grvq.rvqs.0.project_out") {  // residual_vq.py:138, 241
    CAct in(x, nullptr);
    RUN(ensure_planes(h, in, M, c.codebook_dim, ws, s, input_layout(h, h->vq_pout, M, false), 0));
    WS_READY(h, ws, "workspace too small for the module");
    ConvCall co = pointwise(in, M);
    co.y = y;
    return run_conv(h, h->vq_pout, co, s);
  }
  // ConvNeXtBlock (convnext_utils.py:263-282)
  const BlockW* blk = nullptr;
  if (match_idx(m, "encoder.stages.%d.%d%n", &a, &b) && a >= 0 && a < 4 && b >= 0 && b < (int)h->blocks[a].size())
    blk = &h->blocks[a][b];
  else if (m == "quantizer.downsample.0.1") blk = &h->vq_down_blk;
  else if (m == "quantizer.upsample.0.1") blk = &h->vq_up_blk;
  if (blk) {
    if (!blk->C) return fail(h, DCX_ERR_STATE, "module weights not finalized");
    Act ln = conv_input(h, ws, (size_t)M * blk->C);
    Act hid = conv_input(h, ws, (size_t)M * 4 * blk->C);
    row_ranges(h, ws, M, ln, hid);
    WS_READY(h, ws, "workspace too small for the module");
    HIPCHK(h, hipMemcpyAsync(y, x, sizeof(float) * M * blk->C, hipMemcpyDeviceToDevice, s));
    return run_block(h, *blk, y, nullptr, B, L, ln, hid, s);
  }
  // channels-first LayerNorm (convnext_utils.py:186-213)
  const LnW* lw = nullptr;
  if (m == "encoder.downsample_layers.0.1") lw = &h->stem_ln;
  else if (match_idx(m, "encoder.downsample_layers.%d.0%n", &a) && a >= 1 && a < 4) lw = &h->ds_ln[a];
  else if (m == "encoder.norm") lw = &h->enc_norm;
  if (lw) {
    if (ws.dry) return DCX_OK;
    return run_ln(h, *lw, x, Act{y, nullptr}, M, s);
  }
  // nearest-code search on x_pjt_in (EuclideanCodebook.forward, vector_quantize_pytorch.py:496-506)
  if (m == "quantizer.search") {
    if (!h->vq[0].codebook) return fail(h, DCX_ERR_STATE, "module weights not finalized");
    const int CD = c.codebook_dim, NC = c.codebook_size;
    // bf16 mode: the pipeline's search (compact bf16 x_pjt_in for the one-product prefilter, exact fp64
    // rescore of x as given).  The reference searches x.float() with autocast off
    // (vector_quantize_pytorch.py:462-498), x being project_in's bf16 output; row_sqnorm's |x - bf16(x)|^2
    // keeps the prefilter's bound valid for an input that is not bf16-valued.
    const bool x6 = x6_mode(h);
    const Layout xl = vq_xlayout(h);
    const int ntiles = x6 ? dcx::vq_prefilter_ntiles(NC, CD, xl) : dcx::vq_argmin_ntiles(NC);
    unsigned short* P6 = x6 ? ws.u16((size_t)M * CD * 3) : nullptr;
    const VqScratch vs = vq_scratch(h, ws, M, ntiles, x6);
    WS_READY(h, ws, "workspace too small for the module");
    if (x6) LAUNCH(h, s, "split_planes", 0, 10.0 * M * CD, dcx::launch_split_planes(x, P6, M, CD, xl, s));
    return run_vq_search(h, 0, x, P6, xl, M, vs, ntiles, static_cast<int32_t*>(yv), s, h->gemm_mode == DCX_GEMM_BF16);
  }
  if (!h->has_gen && m.rfind("generator.", 0) == 0) return fail(h, DCX_ERR_STATE, "generator weights were not finalized");
  if (m == "generator.conv_pre") {  // generators.py:121
    CAct in(x, nullptr);
    RUN(ensure_planes(h, in, M, c.vq_dim, ws, s, h2_if(takes_h3_conv(h, h->conv_pre, L)), B));
    WS_READY(h, ws, "workspace too small for the module");
    ConvCall cc = framed(in, B, L, c.vq_dim);
    cc.y = y;
    return run_conv(h, h->conv_pre, cc, s);
  }
  if (m == "generator.conv_post") {  // generators.py:141-145: activation_post (SiLU), conv_post, tanh
    int ch = c.gen_channels;
    for (int i = 0; i < c.n_ups; ++i) ch /= 2;
    float* t = ws.f((size_t)M * ch);
    WS_READY(h, ws, "workspace too small for the module");
    LAUNCH(h, s, "silu_act", 0, 8.0 * M * ch, dcx::launch_silu_act(x, t, nullptr, M, ch, s));
    return run_conv_post(h, t, y, B, L, ch, s);
  }
  // ConvTranspose1d (generators.py:118-147, ups[i])
  if (match_idx(m, "generator.ups.%d%n", &a) && a >= 0 && a < c.n_ups) {
    const ConvW& up = h->ups[a];
    CAct in(x, nullptr);
    if (!(x6_mode(h) && f32_input_ok(up))) RUN(ensure_planes(h, in, M, up.cin, ws, s, h2_if(takes_h3_conv(h, up, L)), B));
    WS_READY(h, ws, "workspace too small for the module");
    ConvCall cc = framed(in, B, L, up.cin);
    cc.y = y;
    return run_conv(h, up, cc, s);
  }
  auto in_form = [&](const Act& v, const ConvW& consumer) -> Act { return fp32_form(h, v, consumer); };
  // ResBlock1 (convnext_utils.py:106-113), as per-conv launches of the production conv kernels
  if (match_idx(m, "generator.resblocks.%d.blocks.%d%n", &a, &b) && a >= 0 && a < c.n_ups && b >= 0 && b < c.n_res) {
    const ConvW& w0 = h->res[a][b][0][0];
    const int C = w0.cout;
    Act XS = conv_input(h, ws, (size_t)M * C);  // silu(state), the c1 input (unless silu on load)
    Act Tb = conv_input(h, ws, (size_t)M * C);  // silu(c1 output)
    RangeArena ra;
    ra.reserve(ws, B);
    WS_READY(h, ws, "workspace too small for the module");
    HIPCHK(h, dcx::launch_zero_words(ra.base, (long long)RangeArena::kSlots * B, s));
    const bool silu_on_load = x6_mode(h) && f32_input_ok(w0);
    Act XSi = in_form(XS, w0), Tbi = in_form(Tb, w0);
    XSi.lay = Tbi.lay = h2_if(h3_stage(h, a, L));
    HIPCHK(h, hipMemcpyAsync(y, x, sizeof(float) * M * C, hipMemcpyDeviceToDevice, s));
    RUN(resblock_input(h, y, XSi, silu_on_load, B, L, C, ra, s));
    Rng st = XSi.r;  // the state's range: its measured max |.| (and, in h2, its silu's shift)
    for (int ci = 0; ci < 3; ++ci) {
      const ConvW& w1 = h->res[a][b][ci][0];
      const ConvW& w2 = h->res[a][b][ci][1];
      Act in1 = silu_on_load ? Act{y, nullptr} : XSi;
      in1.r = st;
      ConvCall c1 = framed(in1, B, L, C);
      c1.silu_in = silu_on_load;
      c1.silu_to(Tbi);
      c1.yb = prog_conv(w1, st);
      c1.y_amax = ra.amax();
      c1.y_ash = Tbi.lay == LAYOUT_H2 ? ra.ash() : nullptr;
      RUN(run_conv(h, w1, c1, s));
      const Rng tr{c1.y_ash, 0, c1.y_amax, 0.f};
      Act tin = Tbi;
      tin.r = tr;
      ConvCall c2 = framed(tin, B, L, C);
      c2.epi = dcx::EPI_RES;
      c2.res = y;
      c2.y = y;
      if (!silu_on_load && ci < 2) c2.silu_to(XSi);
      c2.yb.c = w2.b_abs;  // |state + c2 + b2| <= max|state| + g2 max|c1 output| + max|b2|
      prog_add(c2.yb, 1.0f, Rng{nullptr, 0, st.amax, 0.f});
      prog_add(c2.yb, w2.g_abs, tr);
      c2.y_amax = ra.amax();
      c2.y_ash = !silu_on_load && ci < 2 && XSi.lay == LAYOUT_H2 ? ra.ash() : nullptr;
      RUN(run_conv(h, w2, c2, s));
      st = Rng{c2.y_ash, 0, c2.y_amax, 0.f};
    }
    return DCX_OK;
  }
  // ParralelBlock of stage i followed by the generator's SiLU: silu(mean of the ResBlock1s), fp32
  if (match_idx(m, "generator.resblocks.%d%n", &a) && a >= 0 && a < c.n_ups) {
    constexpr int NR = dcx::kMaxGroup;
    const ConvW& w0 = h->res[a][0][0][0];
    const int C = w0.cout;
    const size_t per = (size_t)M * C;
    float* X = ws.f(per);
    Act XS = conv_input(h, ws, per);
    PBlockBufs pb;
    Act RS[NR];
    for (int rb = 0; rb < c.n_res; ++rb) {
      pb.R[rb] = ws.f(per);
      RS[rb] = conv_input(h, ws, per);
      pb.Tb[rb] = conv_input(h, ws, per);
    }
    RangeArena ra;
    ra.reserve(ws, B);
    WS_READY(h, ws, "workspace too small for the module");
    HIPCHK(h, dcx::launch_zero_words(ra.base, (long long)RangeArena::kSlots * B, s));
    const bool silu_on_load = x6_mode(h) && f32_input_ok(w0);
    HIPCHK(h, hipMemcpyAsync(X, x, sizeof(float) * per, hipMemcpyDeviceToDevice, s));
    pb.X = X;
    const Layout lay = h2_if(h3_stage(h, a, L));
    pb.XS = in_form(XS, w0);
    pb.XS.lay = lay;
    for (int rb = 0; rb < c.n_res; ++rb) {
      pb.RS[rb] = in_form(RS[rb], w0);
      pb.Tb_in[rb] = in_form(pb.Tb[rb], w0);
      pb.RS[rb].lay = pb.Tb_in[rb].lay = lay;
    }
    RUN(resblock_input(h, X, pb.XS, silu_on_load, B, L, C, ra, s));
    pb.Mx = y;
    pb.last = true;
    pb.amax_X = pb.XS.r.amax;
    pb.ra = &ra;
    return run_parallel_block(h, a, B, L, pb, s);
  }
  return fail(h, DCX_ERR_INVALID_ARG, "unknown module: " + m);
}

}  // namespace dcx::host
