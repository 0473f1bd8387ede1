// The generator of the host runtime: the ParallelBlocks (fused pairs or grouped per-conv launches)
// with their h3 range bookkeeping, and stage_generate.
#include "dcx_host.h"

namespace dcx::host {

static int max_gen_width(const dcx_config& c) {  // max over generator layers of channels x (L / T)
  int best = c.gen_channels, ch = c.gen_channels, up = 1;
  for (int i = 0; i < c.n_ups; ++i) {
    ch /= 2;
    up *= c.up_rates[i];
    best = std::max(best, ch * up);
  }
  return best;
}

// The fused pair kernel serves a stage when its ResBlock convs are C = 32 / 64 in x6 arithmetic with
// odd kernels, c2 reach <= 8 and c1 reach <= 32 rows, and biases (launch_res_pair checks again).
static bool res_pair_ok(const dcx_codec* h, int stage) {
  if (!h->res_pair || h->gemm_mode != DCX_GEMM_X6) return false;
  const dcx_config& c = h->cfg;
  for (int rb = 0; rb < c.n_res; ++rb)
    for (int ci = 0; ci < 3; ++ci)
      for (int j = 0; j < 2; ++j) {
        const ConvW& w = h->res[stage][rb][ci][j];
        const int hk = (w.taps - 1) / 2;
        if ((w.cout != 32 && w.cout != 64) || w.cin != w.cout || !w.w6 || !w.b || w.taps % 2 == 0 || hk > 8 ||
            w.phases != 1 || w.in_step < 1 || hk * w.in_step > 32 || w.in_base[0] != -hk * w.in_step ||
            (j == 1 && w.in_step != 1))
          return false;
      }
  return true;
}

// Whether generator stage i runs its ResBlock convs in h3 arithmetic (Knobs::h3, x6 mode, not in
// the split-K latency mode, every conv with h3 weights): their inputs are then written in the h2
// layout by their producers (ConvT, c1, c2 epilogues).
// rows: the stage's rows per clip (its ResBlock convs' input length)
bool h3_stage(const dcx_codec* h, int i, long long rows) {
  if (!h->knobs.h3 || h->gemm_mode != DCX_GEMM_X6 || h->split_k >= 2) return false;
  if (!h3_rows_ok(rows, h->res[i][0][0][0].cin)) return false;
  for (int rb = 0; rb < h->cfg.n_res; ++rb)
    for (int j = 0; j < 3; ++j)
      if (!h->res[i][rb][j][0].w3 || !h->res[i][rb][j][1].w3) return false;
  return true;
}

// ParralelBlock.forward (convnext_utils.py:137-138) of generator stage i: three ResBlock1
// (convnext_utils.py:106-113) on X, their mean, and the SiLU that follows it in the generator
// (generators.py:125 / :141), written to b.Mx as fp32 (b.last) or to b.next.  The C = 32 / 64
// stages run as fused pairs (conv_res_pair), the others as grouped per-conv launches.  Every h2
// tensor is range-scaled from a bound over the maxima its producers measured (dcx_kernels.h).
int run_parallel_block(dcx_codec* h, int i, int B, int Lo, const PBlockBufs& b, hipStream_t s) {
  const dcx_config& c = h->cfg;
  constexpr int NR = dcx::kMaxGroup;
  const ConvW& rconv = h->res[i][0][0][0];  // every ResBlock conv of the stage has Cin = Cout = Co
  const int Co = rconv.cout;
  const bool silu_on_load = x6_mode(h) && f32_input_ok(rconv);
  RangeArena& ra = *b.ra;
  if (silu_on_load && res_pair_ok(h, i)) {
    // fused pairs: X -> R[rb] -> Tb[rb] (as fp32) -> silu(ParallelBlock mean)
    float* Ra[NR];
    float* Rb[NR];
    for (int rb = 0; rb < c.n_res; ++rb) {
      Ra[rb] = b.R[rb];
      Rb[rb] = b.Tb[rb].f ? b.Tb[rb].f : reinterpret_cast<float*>(b.Tb[rb].p);
    }
    float* out = b.last ? b.Mx : b.next.f;
    bool h3 = h->knobs.h3_pairs && h->split_k < 2;  // conv_res_pair_h3 (every conv with h3 weights)
    for (int rb = 0; rb < c.n_res; ++rb)
      for (int ci = 0; ci < 3; ++ci) h3 = h3 && h->res[i][rb][ci][0].w3 && h->res[i][rb][ci][1].w3;
    const float* st_amax[NR];  // measured max |state| per clip of each ResBlock's pair input
    for (int rb = 0; rb < c.n_res; ++rb) st_amax[rb] = b.amax_X;
    for (int ci = 0; ci < 3; ++ci) {
      dcx::ResPairParams rp{};
      rp.h3 = h3 ? 1 : 0;
      double fl = 0, by = 0;
      for (int rb = 0; rb < c.n_res; ++rb) {
        const ConvW& w1 = h->res[i][rb][ci][0];
        const ConvW& w2 = h->res[i][rb][ci][1];
        rp.src[rb] = ci == 0 ? b.X : (ci == 1 ? Ra[rb] : Rb[rb]);
        rp.dst[rb] = ci == 0 ? Ra[rb] : (ci == 1 ? Rb[rb] : nullptr);
        rp.w1[rb] = h3 ? w1.w3 : w1.w6;
        rp.w2[rb] = h3 ? w2.w3 : w2.w6;
        rp.w3_shift1[rb] = w1.w3_shift;
        rp.w3_shift2[rb] = w2.w3_shift;
        rp.b1[rb] = w1.b;
        rp.b2[rb] = w2.b;
        rp.taps[rb] = w1.taps;
        rp.dil[rb] = w1.in_step;
        rp.src_amax[rb] = st_amax[rb];
        rp.dst_amax[rb] = ci < 2 ? ra.amax() : nullptr;
        rp.g1[rb] = w1.g_abs;
        rp.bm1[rb] = w1.b_abs;
        ConvCall cc = framed(Act{b.X, nullptr}, B, Lo, Co);
        fl += conv_flops(w1, cc) + conv_flops(w2, cc);
        by += 8.0 * B * Lo * Co;
      }
      rp.nmem = c.n_res;
      rp.mean_out = ci == 2 ? out : nullptr;
      rp.bstride = (long long)Lo * Co;
      rp.L = Lo;
      rp.batch = B;
      rp.C = Co;
      rp.rflag = h->rflag;
      rp.kn = &h->knobs;
      rp.clip_len = b.lens;
      rp.len_mul = b.lens ? Lo / b.frames_max : 1;
      if (b.lens && !h3)
        return fail(h, DCX_ERR_INVALID_ARG, "ragged decode needs the h3 pair kernel (DCX_H3_PAIRS=0 or weights without h3 form)");
      if (h3)
        for (int rb = 0; rb < c.n_res; ++rb)
          if (!rp.src_amax[rb] || (ci < 2 && !rp.dst_amax[rb]))
            return fail(h, DCX_ERR_STATE, "internal: h3 range slots exhausted");
      ProfScope ps(h, s);
      const char* kname = "conv_res_pair";
      HIPCHK(h, dcx::launch_res_pair(rp, s, &kname));
      ps.done(kname, fl, by);
      for (int rb = 0; rb < c.n_res; ++rb) st_amax[rb] = rp.dst_amax[rb];
    }
    return DCX_OK;
  }
  // ranges of each ResBlock's state (its max |.|) and of the c1 inputs in h2
  Rng st[NR], in1[NR];
  for (int rb = 0; rb < c.n_res; ++rb) {
    st[rb].amax = b.amax_X;
    in1[rb] = b.XS.r;
    in1[rb].amax = b.amax_X;
  }
  for (int ci = 0; ci < 3; ++ci) {
    const ConvW* w1[NR];
    ConvCall c1[NR];
    Rng tr[NR];  // silu(c1 output): shift and the measured max |c1 output|
    for (int rb = 0; rb < c.n_res; ++rb) {  // c1 of every ResBlock: one grouped launch
      Act src = silu_on_load ? Act{ci == 0 ? b.X : b.R[rb], nullptr} : (ci == 0 ? b.XS : b.RS[rb]);
      src.r = in1[rb];
      c1[rb] = framed(src, B, Lo, Co);
      c1[rb].ragged(b.lens, b.frames_max);
      c1[rb].silu_in = silu_on_load;
      c1[rb].silu_to(b.Tb_in[rb]);
      w1[rb] = &h->res[i][rb][ci][0];
      c1[rb].yb = prog_conv(*w1[rb], in1[rb]);
      c1[rb].y_amax = ra.amax();
      c1[rb].y_ash = b.Tb_in[rb].lay == LAYOUT_H2 ? ra.ash() : nullptr;
      tr[rb].ash = c1[rb].y_ash;
      tr[rb].amax = c1[rb].y_amax;
    }
    RUN(run_conv_group(h, w1, c1, c.n_res, s));
    if (ci < 2) {  // c2 of every ResBlock: grouped; residual X (first pair) or the block's state
      const ConvW* w2[NR];
      ConvCall c2[NR];
      for (int rb = 0; rb < c.n_res; ++rb) {
        Act tin = b.Tb_in[rb];
        tin.r = tr[rb];
        c2[rb] = framed(tin, B, Lo, Co);
        c2[rb].ragged(b.lens, b.frames_max);
        c2[rb].epi = dcx::EPI_RES;
        c2[rb].res = ci == 0 ? b.X : b.R[rb];
        c2[rb].y = b.R[rb];
        if (!silu_on_load) c2[rb].silu_to(b.RS[rb]);
        w2[rb] = &h->res[i][rb][ci][1];
        // |state + c2 + b2| <= max|state| + g2 max|c1 output| + max|b2|
        c2[rb].yb.c = w2[rb]->b_abs;
        prog_add(c2[rb].yb, 1.0f, st[rb]);
        prog_add(c2[rb].yb, w2[rb]->g_abs, tr[rb]);
        c2[rb].y_amax = ra.amax();
        c2[rb].y_ash = !silu_on_load && b.RS[rb].lay == LAYOUT_H2 ? ra.ash() : nullptr;
      }
      RUN(run_conv_group(h, w2, c2, c.n_res, s));
      for (int rb = 0; rb < c.n_res; ++rb) {
        st[rb] = Rng{};
        st[rb].amax = c2[rb].y_amax;
        in1[rb] = Rng{c2[rb].y_ash, 0, c2[rb].y_amax, 0.f};
      }
    } else {  // last pair: ParallelBlock mean folded into the epilogues, in ResBlock order
      const ConvW* w2[NR];
      ConvCall cm[NR];
      for (int rb = 0; rb < c.n_res; ++rb) {
        ConvCall& cc = cm[rb];
        Act tin = b.Tb_in[rb];
        tin.r = tr[rb];
        cc = framed(tin, B, Lo, Co);
        cc.ragged(b.lens, b.frames_max);
        cc.epi = dcx::EPI_RES;
        cc.res = b.R[rb];
        cc.macc = b.Mx;
        cc.mean = rb == 0 ? dcx::MEAN_FIRST : (rb == c.n_res - 1 ? dcx::MEAN_LAST : dcx::MEAN_MID);
        w2[rb] = &h->res[i][rb][ci][1];
        if (rb == c.n_res - 1) {
          // silu(mean): input of ups[i+1], or (fp32, in place) of conv_post
          if (b.last) cc.y2 = b.Mx;
          else cc.silu_to(b.next);  // input of the next ConvT
          // |mean| <= (1/3) sum over the ResBlocks of (max|state| + g2 max|c1 output| + max|b2|)
          float bc = 0.f;
          for (int m = 0; m < c.n_res; ++m) {
            const ConvW& wm = h->res[i][m][ci][1];
            bc += wm.b_abs / 3.0f;
            prog_add(cc.yb, 1.0f / 3.0f, st[m]);
            prog_add(cc.yb, wm.g_abs / 3.0f, tr[m]);
          }
          cc.yb.c = round_up((double)bc * (1.0 + 1e-6));
          cc.y_amax = b.next_amax;
          cc.y_ash = b.next_ash;
        }
      }
      // split-K mode: one grouped launch and one chained reduce; otherwise conv by conv (the
      // mean's order forbids the grouped unsplit kernel)
      int rc = 1;
      if (h->split_k >= 2 && c.n_res > 1) {
        ConvParams p[NR];
        double fl = 0, by = 0;
        for (int rb = 0; rb < c.n_res; ++rb) {
          RUN(conv_params(h, *w2[rb], cm[rb], false, p[rb]));
          fl += conv_flops(*w2[rb], cm[rb]);
          by += conv_bytes(*w2[rb], cm[rb]);
        }
        rc = run_conv_group_split(h, w2, cm, p, c.n_res, fl, by, s);
      }
      if (rc != 1) RUN(rc);
      else
        for (int rb = 0; rb < c.n_res; ++rb) RUN(run_conv(h, *w2[rb], cm[rb], s));
    }
  }
  if (!ra.ok()) return fail(h, DCX_ERR_STATE, "internal: h3 range slots exhausted");
  return DCX_OK;
}

// a tensor consumed by a small-Cout conv in fp32 (those kernels split while staging), range kept
Act fp32_form(dcx_codec* h, const Act& a, const ConvW& consumer) {
  if (!x6_mode(h) || !f32_input_ok(consumer)) return a;
  Act f{a.f ? a.f : reinterpret_cast<float*>(a.p), nullptr};
  f.r = a.r;
  return f;
}

// conv_post and tanh (generators.py:142-145) on x = silu(the last stage's mean) [B][L][C]
int run_conv_post(dcx_codec* h, const float* x, float* wav, int B, int L, int C, hipStream_t s, const int* lens,
                  int len_mul) {
  const int k = h->cfg.gen_post_k;
  const bool bf = h->gemm_mode == DCX_GEMM_BF16;
  LAUNCH(h, s, "conv_post_tanh", 2.0 * B * L * C * k, 4.0 * B * L * (C + 1),
         dcx::launch_conv_post_tanh(x, h->post_w, bf ? bf16_f(bf16_rne(h->post_b)) : h->post_b, wav, B, L, C, k,
                                    bf ? 1 : 0, s, lens, len_mul));
  return DCX_OK;
}

// Ragged batches (lens, dcx_generate_ragged): the memory layout, the workspace plan and every choice
// of a kernel family or tile (big_tiles_pay, h3_stage, takes_h3_conv, the pair launcher's tile height)
// follow B and T, the padded frame count, never the lengths, which only the device sees: one captured
// graph serves any lengths, and a clip's kernels do not depend on its neighbours' lengths.  Every
// producer writes zeros from a clip's length to the padded end (ConvParams::clip_len), so every
// consumer reads the clip's own zero padding; z is bounded where it is split (launch_h2_ranged).
int stage_generate(dcx_codec* h, CAct z, int B, int T, float* wav, Bump& ws, hipStream_t s, const int* lens) {
  const dcx_config& c = h->cfg;
  if (lens && !ws.dry) {
    if (h->gemm_mode != DCX_GEMM_X6)
      return fail(h, DCX_ERR_INVALID_ARG, "ragged decode runs in DCX_GEMM_X6 (the other modes' kernels are not length-aware)");
    if (z.p || !takes_h3_conv(h, h->conv_pre, T))
      return fail(h, DCX_ERR_INVALID_ARG, "ragged decode needs conv_pre in h3 arithmetic (DCX_H3=0: z would be split unbounded)");
  }
  // z in conv_pre's h2 form, range-scaled by each clip's exact max (the fused pipeline's z as well)
  RUN(ensure_planes(h, z, (long long)B * T, c.vq_dim, ws, s, h2_if(takes_h3_conv(h, h->conv_pre, T)), B, lens));
  const size_t per = (size_t)B * T * max_gen_width(c);
  // The ParallelBlock's ResBlocks are independent until the mean, so each keeps its own state and
  // the convs of one dilation index run as one grouped launch (run_conv_group).
  constexpr int NR = dcx::kMaxGroup;
  if (c.n_res > NR) return fail(h, DCX_ERR_INVALID_ARG, "more ResBlocks per stage than supported");
  if (2 + 36 * c.n_ups > RangeArena::kSlots) return fail(h, DCX_ERR_INVALID_ARG, "too many generator stages");
  float* X = ws.f(per);   // ConvT output (residual of each ResBlock's first pair)
  float* Mx = ws.f(per);  // ParallelBlock mean accumulator; silu(mean) of the last stage
  Act S = conv_input(h, ws, per);   // silu(stage input) -> ConvT
  Act XS = conv_input(h, ws, per);  // silu(X)
  float* R[NR];                     // ResBlock states
  Act RS[NR], Tb[NR];               // silu(R), silu(c1 output)
  for (int rb = 0; rb < c.n_res; ++rb) {
    R[rb] = ws.f(per);
    RS[rb] = conv_input(h, ws, per);
    Tb[rb] = conv_input(h, ws, per);
  }
  RangeArena ra;
  ra.reserve(ws, B);
  WS_READY(h, ws, "workspace too small for generate");
  // the measured maxima only serve h3 consumers: none in the split-K latency mode or the fp32 mode,
  // where the epilogues then skip their range reductions and no slot is cleared (C5: one launch and
  // the reductions of ~40 epilogues per hop)
#ifndef DCX_DIAG_LAT_RANGES  // A/B build: the slots tracked in every mode (round-6 first form)
  if (!x6_mode(h) || h->split_k >= 2) ra.base = nullptr;
#endif
  if (ra.base) HIPCHK(h, dcx::launch_zero_words(ra.base, (long long)RangeArena::kSlots * B, s));
  // Tensors consumed by small-Cout convs are kept in fp32 (those kernels split them while
  // staging: the stages are bound by HBM traffic, and planes cost 6 B per element against 4).
  auto in_form = [&](const Act& a, const ConvW& consumer) -> Act { return fp32_form(h, a, consumer); };
  int C = c.gen_channels, L = T;
  {  // conv_pre, then the first stage's SiLU (generators.py:121,125) fused as the only output
    ConvCall cc = framed(z, B, T, c.vq_dim);
    cc.ragged(lens, T);
    Act S0 = S;
    S0.lay = h2_if(S.p && takes_h3_conv(h, h->ups[0], T));
    cc.silu_to(S0);
    cc.yb = prog_conv(h->conv_pre, z.r);
    cc.y_amax = ra.amax();
    cc.y_ash = S0.lay == LAYOUT_H2 ? ra.ash() : nullptr;
    RUN(run_conv(h, h->conv_pre, cc, s));
    S.r = Rng{cc.y_ash, 0, cc.y_amax, 0.f};
  }
  for (int i = 0; i < c.n_ups; ++i) {
    const ConvW& up = h->ups[i];
    const int Co = up.cout, Lo = L * c.up_rates[i];
    const ConvW& rconv = h->res[i][0][0][0];  // every ResBlock conv of the stage has Cin = Cout = Co
    Act S_i = in_form(S, up);
    S_i.lay = h2_if(S_i.p && takes_h3_conv(h, up, L));  // as conv_pre / the previous stage's mean epilogue wrote it
    Act XS_i = in_form(XS, rconv);
    Act RS_i[NR], Tb_i[NR];
    for (int rb = 0; rb < c.n_res; ++rb) {
      RS_i[rb] = in_form(RS[rb], rconv);
      Tb_i[rb] = in_form(Tb[rb], rconv);
    }
    // fp32-input stages: the first conv of each pair applies silu to X / R while staging, so
    // silu(X) and silu(R) are never written (7 activation tensors per stage less HBM traffic)
    const bool silu_on_load = x6_mode(h) && f32_input_ok(rconv);
    if (h3_stage(h, i, Lo)) {  // the ResBlock convs' inputs in the h2 layout (conv_gemm_x3dq)
      XS_i.lay = LAYOUT_H2;
      for (int rb = 0; rb < c.n_res; ++rb) RS_i[rb].lay = Tb_i[rb].lay = LAYOUT_H2;
    }
    float* amax_X = ra.amax();
    {
      ConvCall cc = framed(S_i, B, L, C);
      cc.ragged(lens, T);
      cc.y = X;
      if (!silu_on_load) cc.silu_to(XS_i);
      cc.yb = prog_conv(up, S_i.r);
      cc.y_amax = amax_X;
      cc.y_ash = !silu_on_load && XS_i.lay == LAYOUT_H2 ? ra.ash() : nullptr;
      RUN(run_conv(h, up, cc, s));
      XS_i.r = Rng{cc.y_ash, 0, amax_X, 0.f};
    }
    PBlockBufs pb;
    pb.X = X;
    pb.XS = XS_i;
    for (int rb = 0; rb < c.n_res; ++rb) {
      pb.R[rb] = R[rb];
      pb.RS[rb] = RS_i[rb];
      pb.Tb[rb] = Tb[rb];
      pb.Tb_in[rb] = Tb_i[rb];
    }
    pb.Mx = Mx;
    pb.last = i == c.n_ups - 1;
    pb.amax_X = amax_X;
    pb.ra = &ra;
    pb.lens = lens;
    pb.frames_max = T;
    if (!pb.last) {
      pb.next = in_form(S, h->ups[i + 1]);
      pb.next.lay = h2_if(pb.next.p && takes_h3_conv(h, h->ups[i + 1], Lo));
      pb.next_amax = ra.amax();
      pb.next_ash = pb.next.lay == LAYOUT_H2 ? ra.ash() : nullptr;
    }
    if (!ra.ok()) return fail(h, DCX_ERR_STATE, "internal: h3 range slots exhausted");
    RUN(run_parallel_block(h, i, B, Lo, pb, s));
    S.r = Rng{pb.next_ash, 0, pb.next_amax, 0.f};
    C = Co;
    L = Lo;
  }
  return run_conv_post(h, Mx, wav, B, L, C, s, lens, L / T);
}

}  // namespace dcx::host
