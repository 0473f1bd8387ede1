// Checkpoint ingestion of the host runtime: weight-norm folding (fp64), packing into the kernels'
// layouts, the mel front end's bases, the decode tables, the h3 range bounds of every conv.
#include "dcx_host.h"
#include "dcx_w3_layout.h"

namespace dcx::host {

struct Err {
  int code;
  std::string msg;
};

// ----------------------------------------------------------------------------------------
// weight ingestion
// ----------------------------------------------------------------------------------------
static const HostTensor* find(dcx_codec* h, const std::string& k) {
  auto it = h->host.find(k);
  return it == h->host.end() ? nullptr : &it->second;
}

// Effective weight, folding weight norm (torch._weight_norm(v, g, dim=0)) in fp64.
static bool get_weight(dcx_codec* h, const std::string& prefix, HostTensor& out) {
  if (auto t = find(h, prefix + ".weight")) {
    out = *t;
    return true;
  }
  const char* pairs[2][2] = {{".parametrizations.weight.original0", ".parametrizations.weight.original1"},
                             {".weight_g", ".weight_v"}};
  for (auto& pr : pairs) {
    auto g = find(h, prefix + pr[0]);
    auto v = find(h, prefix + pr[1]);
    if (g && v) {
      out.shape = v->shape;
      out.data.resize(v->data.size());
      const int64_t d0 = v->shape[0], inner = v->numel() / d0;
      if ((int64_t)g->data.size() != d0) return false;
      for (int64_t i = 0; i < d0; ++i) {
        double nrm = 0;
        for (int64_t j = 0; j < inner; ++j) nrm += (double)v->data[i * inner + j] * v->data[i * inner + j];
        nrm = std::sqrt(nrm);
        const double sc = (double)g->data[i] / nrm;
        for (int64_t j = 0; j < inner; ++j) out.data[i * inner + j] = (float)(sc * v->data[i * inner + j]);
      }
      return true;
    }
  }
  return false;
}

// x = hi + mid + lo, the same split the x6 kernel applies to activations.
static void split3_host(float x, unsigned short& h, unsigned short& m, unsigned short& l) {
  h = bf16_rne(x);
  const float r1 = x - bf16_f(h);
  m = bf16_rne(r1);
  const float r2 = r1 - bf16_f(m);
  l = bf16_rne(r2);
}

// a double rounded up to float (range bounds stay upper bounds)
float round_up(double v) {
  float f = (float)v;
  if ((double)f < v) f = std::nextafter(f, INFINITY);
  return f;
}

struct Builder {
  dcx_codec* h;
  bool dry;  // validate names and shapes only: no device allocation
  Err e{DCX_OK, ""};

  bool bad() const { return e.code != DCX_OK; }
  void set(int c, const std::string& m) {
    if (!bad()) e = {c, m};
  }

  void* upload_raw(const void* src, size_t bytes, const char* what = "weights") {
    if (bad() || dry) return nullptr;
    void* p = nullptr;
    if (hipMalloc(&p, bytes + 16) != hipSuccess) {
      set(DCX_ERR_OOM, std::string("hipMalloc failed while uploading ") + what);
      return nullptr;
    }
    h->allocs.push_back(p);
    if (hipMemcpy(p, src, bytes, hipMemcpyHostToDevice) != hipSuccess) {
      set(DCX_ERR_HIP, std::string("hipMemcpy failed while uploading ") + what);
      return nullptr;
    }
    return p;
  }
  float* upload(const std::vector<float>& v) { return (float*)upload_raw(v.data(), v.size() * sizeof(float)); }
  unsigned short* upload16(const std::vector<unsigned short>& v) {
    return (unsigned short*)upload_raw(v.data(), v.size() * sizeof(unsigned short), "split weights");
  }
  // fp32 packed [phases][cout][taps][cin] -> x6 layout [phase][tap][cin/16][cout][2][3][8] bf16
  unsigned short* split_pack(const std::vector<float>& pk, int phases, int cout, int taps, int cin) {
    if (bad() || dry) return nullptr;
    const int nch = cin / 16;
    std::vector<unsigned short> out((size_t)phases * taps * nch * cout * 48);
    for (int r = 0; r < phases; ++r)
      for (int m = 0; m < taps; ++m)
        for (int c = 0; c < nch; ++c)
          for (int o = 0; o < cout; ++o) {
            unsigned short* dst = &out[((((size_t)r * taps + m) * nch + c) * cout + o) * 48];
            const float* src = &pk[(((size_t)r * cout + o) * taps + m) * cin + c * 16];
            for (int hh = 0; hh < 2; ++hh)
              for (int j = 0; j < 8; ++j) {
                unsigned short a, b2, c2;
                split3_host(src[hh * 8 + j], a, b2, c2);
                dst[hh * 24 + 0 + j] = a;
                dst[hh * 24 + 8 + j] = b2;
                dst[hh * 24 + 16 + j] = c2;
              }
          }
    return upload16(out);
  }
  // fp32 packed [phases][cout][taps][cin] -> the h3 weights, fp16 h / l of w * 2^shift at w3_offset
  // (dcx_w3_layout.h: steps in [phase][tap][cin/32] order, a step's cout * 64 halves in the flavour
  // cout selects), shift putting the largest |w| in [2^14, 2^15) (conv_gemm_x3dq / x3dw, the pair kernels)
  unsigned short* h2_pack(const std::vector<float>& pk, int phases, int cout, int taps, int cin, int& shift) {
    if (bad() || dry) return nullptr;
    float mx = 0.f;
    for (float v : pk) mx = std::max(mx, std::fabs(v));
    int e = 0;
    if (mx > 0.f) std::frexp(mx, &e);  // mx = f * 2^e, f in [0.5, 1)
    shift = mx > 0.f ? 15 - e : 0;
    std::vector<unsigned short> out((size_t)phases * taps * cin * cout * 2);
    for (int r = 0; r < phases; ++r)
    for (int m = 0; m < taps; ++m)
      for (int o = 0; o < cout; ++o) {
        const float* src = &pk[(((size_t)r * cout + o) * taps + m) * cin];
        for (int j = 0; j < cin; ++j) {
          const float x = std::ldexp(src[j], shift);
          const _Float16 hh = (_Float16)x;
          const _Float16 ll = (_Float16)(x - (float)hh);
          out[(size_t)w3_offset(taps, cin, cout, r, m, j, o, 0)] = __builtin_bit_cast(unsigned short, hh);
          out[(size_t)w3_offset(taps, cin, cout, r, m, j, o, 1)] = __builtin_bit_cast(unsigned short, ll);
        }
      }
    return upload16(out);
  }
  // fp32 packed [cout][cin] (one tap, one phase) -> [cin/32][cout][32] bf16 hi (conv_gemm_bf16dm)
  unsigned short* compact_pack(const std::vector<float>& pk, int cout, int cin) {
    if (bad() || dry) return nullptr;
    std::vector<unsigned short> out((size_t)cout * cin);
    for (int st = 0; st < cin / 32; ++st)
      for (int o = 0; o < cout; ++o)
        for (int j = 0; j < 32; ++j) out[((size_t)st * cout + o) * 32 + j] = bf16_rne(pk[(size_t)o * cin + st * 32 + j]);
    return upload16(out);
  }
  float* alloc(size_t n) {
    if (bad() || dry) return nullptr;
    void* p = nullptr;
    if (hipMalloc(&p, n * sizeof(float) + 16) != hipSuccess) {
      set(DCX_ERR_OOM, "hipMalloc failed");
      return nullptr;
    }
    h->allocs.push_back(p);
    return (float*)p;
  }

  const HostTensor* need(const std::string& k, std::vector<int64_t> shape) {
    auto t = find(h, k);
    if (!t) {
      set(DCX_ERR_MISSING_WEIGHT, "missing checkpoint tensor '" + k + "'");
      return nullptr;
    }
    if (t->numel() != [&] { int64_t n = 1; for (auto s : shape) n *= s; return n; }()) {
      set(DCX_ERR_INVALID_ARG, "checkpoint tensor '" + k + "' has the wrong number of elements");
      return nullptr;
    }
    return t;
  }
  float* vec(const std::string& k, int64_t n) {
    auto t = need(k, {n});
    return t ? upload(t->data) : nullptr;
  }
  // the same vector rounded to bf16 values (fp32 storage)
  float* vec_bf16(const std::string& k, int64_t n) {
    auto t = need(k, {n});
    if (!t) return nullptr;
    std::vector<float> r(t->data.size());
    for (size_t i = 0; i < r.size(); ++i) r[i] = bf16_f(bf16_rne(t->data[i]));
    return upload(r);
  }
  HostTensor weight(const std::string& prefix, std::vector<int64_t> shape) {
    HostTensor w;
    if (bad()) return w;
    if (!get_weight(h, prefix, w)) {
      set(DCX_ERR_MISSING_WEIGHT, "missing checkpoint weight '" + prefix + "'");
      return w;
    }
    int64_t n = 1;
    for (auto s : shape) n *= s;
    if (w.numel() != n) set(DCX_ERR_INVALID_ARG, "checkpoint weight '" + prefix + "' has the wrong shape");
    return w;
  }

  // h3 range bounds of a conv (ConvW::g_abs, b_abs) from its packed fp32 weights [phases][cout][kk]
  // and its bias
  void range_of(ConvW& c, const std::vector<float>& pk, int phases, int cout, size_t kk, const std::string& bias) {
    if (dry) return;
    double g = 0;
    for (int r = 0; r < phases; ++r)
      for (int o = 0; o < cout; ++o) {
        double sacc = 0;
        const float* row = &pk[((size_t)r * cout + o) * kk];
        for (size_t j = 0; j < kk; ++j) sacc += std::fabs((double)row[j]);
        g = std::max(g, sacc);
      }
    c.g_abs = round_up(g);
    double bm = 0;
    if (const HostTensor* t = bias.empty() ? nullptr : find(h, bias))
      for (float v : t->data) bm = std::max(bm, std::fabs((double)v));
    c.b_abs = round_up(bm);
  }

  // Conv1d / Linear weight [Cout][Cin][k] -> packed [Cout][k][Cin].
  // h3: also the h3 weights (conv_gemm_x3dq; the generator's ResBlock convs of the wide stages)
  ConvW conv(const std::string& prefix, int cin, int cout, int k, int dil, int pad, bool has_bias = true,
             bool h3 = false) {
    ConvW c;
    c.cin = cin; c.cout = cout; c.taps = k; c.in_step = dil; c.in_base[0] = -pad;
    HostTensor w = weight(prefix, {cout, cin, k});
    if (bad()) return c;
    std::vector<float> pk((size_t)cout * k * cin);
    for (int o = 0; o < cout; ++o)
      for (int i = 0; i < cin; ++i)
        for (int j = 0; j < k; ++j) pk[((size_t)o * k + j) * cin + i] = w.data[((size_t)o * cin + i) * k + j];
    c.w = upload(pk);
    if (cin % 16 == 0) c.w6 = split_pack(pk, 1, cout, k, cin);
    if (k == 1 && cin % 32 == 0) c.wc = compact_pack(pk, cout, cin);
    if (h3 && cin % 32 == 0) c.w3 = h2_pack(pk, 1, cout, k, cin, c.w3_shift);
    if (has_bias) {
      c.b = vec(prefix + ".bias", cout);
      c.b16 = vec_bf16(prefix + ".bias", cout);
    }
    range_of(c, pk, 1, cout, (size_t)k * cin, has_bias ? prefix + ".bias" : "");
    return c;
  }

  // ConvTranspose1d weight [Cin][Cout][k], stride s, padding (k-s)/2 -> s polyphase convs:
  // output o = q*s + r reads input q + base_r - m with tap j = (r+p)%s + m*s, m < k/s.
  ConvW convT(const std::string& prefix, int cin, int cout, int k, int s, bool h3 = false) {
    ConvW c;
    const int p = (k - s) / 2, taps = k / s;
    c.cin = cin; c.cout = cout; c.taps = taps; c.phases = s; c.in_step = -1; c.out_mul = s;
    HostTensor w = weight(prefix, {cin, cout, k});
    if (bad()) return c;
    std::vector<float> pk((size_t)s * cout * taps * cin);
    for (int r = 0; r < s; ++r) {
      const int jr = (r + p) % s;
      c.in_base[r] = (r + p - jr) / s;
      for (int o = 0; o < cout; ++o)
        for (int m = 0; m < taps; ++m)
          for (int i = 0; i < cin; ++i)
            pk[(((size_t)r * cout + o) * taps + m) * cin + i] = w.data[((size_t)i * cout + o) * k + jr + m * s];
    }
    c.w = upload(pk);
    if (cin % 16 == 0) c.w6 = split_pack(pk, s, cout, taps, cin);
    if (h3 && cin % 32 == 0) c.w3 = h2_pack(pk, s, cout, taps, cin, c.w3_shift);
    c.b = vec(prefix + ".bias", cout);
    c.b16 = vec_bf16(prefix + ".bias", cout);
    range_of(c, pk, s, cout, (size_t)taps * cin, prefix + ".bias");
    return c;
  }

  LnW ln(const std::string& prefix, int C) {
    LnW l;
    l.C = C;
    l.w = vec(prefix + ".weight", C);
    l.b = vec(prefix + ".bias", C);
    return l;
  }

  BlockW block(const std::string& p, int C) {
    BlockW b;
    b.C = C;
    auto dw = need(p + ".dwconv.weight", {C, 1, 7});
    if (dw) {
      std::vector<float> pk((size_t)7 * C);
      for (int c = 0; c < C; ++c)
        for (int j = 0; j < 7; ++j) pk[(size_t)j * C + c] = dw->data[(size_t)c * 7 + j];
      b.dww = upload(pk);
    }
    b.dwb = vec(p + ".dwconv.bias", C);
    b.ln = ln(p + ".norm", C);
    b.pw1 = conv(p + ".pwconv1", C, 4 * C, 1, 1, 0, true, true);
    b.pw2 = conv(p + ".pwconv2", 4 * C, C, 1, 1, 0, true, true);
    b.gamma = vec(p + ".gamma", C);
    return b;
  }
};

// Slaney mel filterbank (torchaudio melscale_fbanks norm='slaney', mel_scale='slaney').
static double hz_to_mel(double f) {
  const double f_sp = 200.0 / 3, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp, logstep = std::log(6.4) / 27.0;
  return f >= min_log_hz ? min_log_mel + std::log(f / min_log_hz) / logstep : f / f_sp;
}
static double mel_to_hz(double m) {
  const double f_sp = 200.0 / 3, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp, logstep = std::log(6.4) / 27.0;
  return m >= min_log_mel ? min_log_hz * std::exp(logstep * (m - min_log_mel)) : f_sp * m;
}
static std::vector<double> mel_fb(int n_freqs, double fmin, double fmax, int n_mels, int sr) {
  std::vector<double> fb((size_t)n_freqs * n_mels, 0.0);
  std::vector<double> f_pts(n_mels + 2);
  const double m0 = hz_to_mel(fmin), m1 = hz_to_mel(fmax);
  for (int i = 0; i < n_mels + 2; ++i) f_pts[i] = mel_to_hz(m0 + (m1 - m0) * i / (n_mels + 1));
  for (int k = 0; k < n_freqs; ++k) {
    const double f = (double)(sr / 2) * k / (n_freqs - 1);
    for (int m = 0; m < n_mels; ++m) {
      const double down = (f - f_pts[m]) / (f_pts[m + 1] - f_pts[m]);
      const double up = (f_pts[m + 2] - f) / (f_pts[m + 2] - f_pts[m + 1]);
      double v = std::max(0.0, std::min(down, up));
      v *= 2.0 / (f_pts[m + 2] - f_pts[m]);
      fb[(size_t)k * n_mels + m] = v;
    }
  }
  return fb;
}

static int build_all(dcx_codec* h, Builder& B, int32_t with_generator) {
  const dcx_config& c = h->cfg;
  // ---- mel front end: DFT basis as a 4-tap conv over 256-sample rows ------------------
  {
    const int N = c.n_fft, nb = N / 2 + 1;
    std::vector<double> win(N);
    for (int n = 0; n < N; ++n) win[n] = 0.5 - 0.5 * std::cos(2.0 * M_PI * n / N);  // hann, periodic
    std::vector<float> basis((size_t)N * N, 0.f);  // [col][n]; cols: re 0..512, im 1..511
    for (int k = 0; k < nb; ++k)
      for (int n = 0; n < N; ++n) {
        const long long kn = ((long long)k * n) % N;
        basis[(size_t)k * N + n] = (float)(win[n] * std::cos(2.0 * M_PI * kn / N));
        if (k > 0 && k < nb - 1) basis[(size_t)(nb + k - 1) * N + n] = (float)(-win[n] * std::sin(2.0 * M_PI * kn / N));
      }
    h->dft.cin = c.hop; h->dft.cout = N; h->dft.taps = N / c.hop; h->dft.in_step = 1;
    h->dft.w = B.upload(basis);
    h->dft.w6 = B.split_pack(basis, 1, N, N / c.hop, c.hop);
    h->dft1 = h->dft;  // [Cout][tap * hop + ci] = [Cout][n]: one tap over whole frames
    h->dft1.cin = N;
    h->dft1.taps = 1;
    const int kpad = (nb + 31) / 32 * 32;  // even number of 16-deep chunks (x6 kernels step in pairs)
    std::vector<double> fb = mel_fb(nb, c.f_min, c.f_max, c.n_mels, c.sample_rate);
    std::vector<float> pk((size_t)c.n_mels * kpad, 0.f);
    for (int m = 0; m < c.n_mels; ++m)
      for (int k = 0; k < nb; ++k) pk[(size_t)m * kpad + k] = (float)fb[(size_t)k * c.n_mels + m];
    h->melfb.cin = kpad; h->melfb.cout = c.n_mels; h->melfb.taps = 1;
    h->melfb.w = B.upload(pk);
    h->melfb.w6 = B.split_pack(pk, 1, c.n_mels, 1, kpad);
  }
  // ---- encoder --------------------------------------------------------------------------
  {
    const std::string e = "encoder.";
    h->stem = B.conv(e + "downsample_layers.0.0", c.n_mels, c.enc_dims[0], 7, 1, 3);
    h->stem1 = h->stem;  // one tap over rows unfolded per clip (launch_ragged_unfold)
    h->stem1.cin = h->stem.taps * h->stem.cin;
    h->stem1.taps = 1;
    h->stem1.in_base[0] = 0;
    h->stem_ln = B.ln(e + "downsample_layers.0.1", c.enc_dims[0]);
    for (int i = 0; i < 4; ++i) {
      if (i > 0) {
        const std::string p = e + "downsample_layers." + std::to_string(i);
        h->ds_ln[i] = B.ln(p + ".0", c.enc_dims[i - 1]);
        h->ds_conv[i] = B.conv(p + ".1", c.enc_dims[i - 1], c.enc_dims[i], 1, 1, 0, true, true);  // + h3 weights
      }
      h->blocks[i].clear();
      for (int j = 0; j < c.enc_depths[i]; ++j)
        h->blocks[i].push_back(B.block(e + "stages." + std::to_string(i) + "." + std::to_string(j), c.enc_dims[i]));
    }
    h->enc_norm = B.ln(e + "norm", c.enc_dims[3]);
  }
  // ---- quantizer ------------------------------------------------------------------------
  {
    const std::string q = "quantizer.";
    const int D = c.vq_dim, CD = c.codebook_dim, NC = c.codebook_size;
    h->vq_down = B.conv(q + "downsample.0.0", D, D, 1, 1, 0, true, true);  // + h3 weights
    h->vq_down_blk = B.block(q + "downsample.0.1", D);
    h->vq_up = B.convT(q + "upsample.0.0", D, D, 1, 1);
    h->vq_up_blk = B.block(q + "upsample.0.1", D);
    h->vq_pin = B.conv(q + "grvq.rvqs.0.project_in", D, CD, 1, 1, 0, true, true);  // + h3 weights
    h->vq_pout = B.conv(q + "grvq.rvqs.0.project_out", CD, D, 1, 1, 0);
    const ConvW& pout = h->vq_pout;
    const int R = h->n_layers;
    h->vq_stats = (int*)B.upload(std::vector<float>(2, 0.f));  // zero counters
    // every layer of the chain: a missing codebook fails the load (never a shorter chain)
    for (int k = 0; k < R; ++k) {
      auto emb = B.need(q + "grvq.rvqs.0.layers." + std::to_string(k) + "._codebook.embed", {1, NC, CD});
      if (!emb) break;
      dcx_codec::VqLayer& L = h->vq[k];
      std::vector<float> e2(NC);
      std::vector<double> e2d(NC);
      double e2m = 0;
      for (int i = 0; i < NC; ++i) {
        double sacc = 0;
        for (int d = 0; d < CD; ++d) sacc += (double)emb->data[(size_t)i * CD + d] * emb->data[(size_t)i * CD + d];
        e2[i] = (float)sacc;
        e2d[i] = sacc;
        e2m = std::max(e2m, sacc);
      }
      L.e2d = (double*)B.upload_raw(e2d.data(), e2d.size() * sizeof(double));
      // rounded up so the prefilter bound stays an upper bound
      L.e2max = std::nextafter((float)e2m, INFINITY);
      L.emax = std::nextafter((float)std::sqrt(e2m), INFINITY);
      L.codebook = B.upload(emb->data);
      L.codebook6 = B.split_pack(emb->data, 1, NC, 1, CD);
      L.e2 = B.upload(e2);
      // max |e - bf16(e)| in fp64, rounded up (vq_prefilter_b1's bound)
      double d2m = 0;
      for (int i = 0; i < NC; ++i) {
        double sacc = 0;
        for (int d = 0; d < CD; ++d) {
          const float v = emb->data[(size_t)i * CD + d];
          const double r = (double)v - (double)bf16_f(bf16_rne(v));
          sacc += r * r;
        }
        d2m = std::max(d2m, sacc);
      }
      L.dmax = std::nextafter((float)(std::sqrt(d2m) * (1.0 + 1e-12)), INFINITY);
      if (dcx::vq_b1_takes(NC, CD)) L.codebook_b1 = B.compact_pack(emb->data, NC, CD);
    }
    float* const codebook = h->vq[0].codebook;
    // A chain decodes by gather-sum and the project_out conv (stage_vq_decode), in the reference's
    // order; only one codebook has a table of its project_out rows.
    if (R == 1) {
      // decode table: project_out applied to every code once, E * W_out^T + b_out.  Row NC holds
      // project_out(0) = b_out, the row of the reference's masked code -1 (residual_vq.py:120-127:
      // masked_fill(-1 -> 0), gather, then the gathered vector zeroed before project_out).
      h->ptable = B.alloc((size_t)(NC + 1) * D);
      h->ptable6 = (unsigned short*)B.alloc((size_t)(NC + 1) * D * 3 / 2);
      if (!B.bad() && !B.dry) {
        // built once with the fp32 MFMA path (the codebook is not held as activation planes)
        ConvCall cp = pointwise(CAct(codebook, nullptr), NC);
        cp.y = h->ptable;
        int rc = run_conv(h, pout, cp, 0, /*force_f32=*/true);
        if (rc != DCX_OK) return rc;
        if (hipMemcpy(h->ptable + (size_t)NC * D, pout.b, sizeof(float) * D, hipMemcpyDeviceToDevice) != hipSuccess ||
            dcx::launch_split_planes(h->ptable, h->ptable6, NC + 1, D, LAYOUT_PLANES, 0) != hipSuccess ||
            hipDeviceSynchronize() != hipSuccess)
          return fail(h, DCX_ERR_HIP, "decode-table build failed");
      }
      // The bf16 mode's table: project_out under the reference's autocast (residual_vq.py:138 inside
      // distil_codec.py:590), bf16(bf16(E) W_out16^T + b_out16) by the one-product conv on the codebook
      // as activation planes (scratch); row NC = bf16(b_out) (the masked code).  Built in a scratch fp32
      // table, then split.
      h->ptable6b = (unsigned short*)B.alloc((size_t)(NC + 1) * D * 3 / 2);
      if (!B.bad() && !B.dry && codebook) {
        float* tmp = nullptr;
        unsigned short* e6 = nullptr;
        if (hipMalloc(&tmp, sizeof(float) * (size_t)(NC + 1) * D) != hipSuccess) return fail(h, DCX_ERR_OOM, "hipMalloc failed");
        if (hipMalloc(&e6, sizeof(unsigned short) * 3 * (size_t)NC * CD) != hipSuccess) {
          hipFree(tmp);
          return fail(h, DCX_ERR_OOM, "hipMalloc failed");
        }
        int rc = dcx::launch_split_planes(codebook, e6, NC, CD, LAYOUT_PLANES, 0) == hipSuccess
                     ? DCX_OK : fail(h, DCX_ERR_HIP, "codebook split failed");
        const int mode = h->gemm_mode;
        h->gemm_mode = DCX_GEMM_BF16;
        ConvCall cp = pointwise(CAct(codebook, e6), NC);
        cp.y = tmp;
        if (rc == DCX_OK) rc = run_conv(h, pout, cp, 0);
        h->gemm_mode = mode;
        if (rc == DCX_OK &&
            (hipMemcpy(tmp + (size_t)NC * D, pout.b16, sizeof(float) * D, hipMemcpyDeviceToDevice) != hipSuccess ||
             dcx::launch_split_planes(tmp, h->ptable6b, NC + 1, D, LAYOUT_PLANES, 0) != hipSuccess || hipDeviceSynchronize() != hipSuccess))
          rc = fail(h, DCX_ERR_HIP, "bf16 decode-table build failed");
        hipFree(e6);
        hipFree(tmp);
        if (rc != DCX_OK) return rc;
      }
    }
    // the h3 range flags (round 6)
    if (!B.bad() && !B.dry) {
      h->rflag = (int*)B.alloc(1);
      if (!h->rflag || hipMemset(h->rflag, 0, sizeof(int)) != hipSuccess) return fail(h, DCX_ERR_HIP, "range flag");
    }
  }
  // ---- generator ------------------------------------------------------------------------
  if (with_generator) {
    const std::string g = "generator.";
    int ch = c.gen_channels;
    // h3 weights for the convs conv_gemm_x3dw takes (Cout % 256 == 0, or Cout % 128 == 0 on its
    // 384 x 128 tiles; two taps or more)
    h->conv_pre = B.conv(g + "conv_pre", c.vq_dim, ch, c.gen_pre_k, 1, (c.gen_pre_k - 1) / 2, true,
                         ch % 256 == 0 && c.gen_pre_k >= 2);
    for (int i = 0; i < c.n_ups; ++i) {
      h->ups[i] = B.convT(g + "ups." + std::to_string(i), ch, ch / 2, c.up_kernels[i], c.up_rates[i],
                          (ch / 2) % 128 == 0 && c.up_kernels[i] / c.up_rates[i] >= 2);
      ch /= 2;
      for (int rb = 0; rb < c.n_res; ++rb) {
        const int k = c.res_kernels[rb];
        for (int j = 0; j < 3; ++j) {
          const int d = c.res_dilations[rb][j];
          const std::string p = g + "resblocks." + std::to_string(i) + ".blocks." + std::to_string(rb);
          const bool h3 = ch % 32 == 0;  // conv_gemm_x3dq / x3dw tiles (C >= 128), conv_res_pair_h3 (32 / 64)
          h->res[i][rb][j][0] = B.conv(p + ".convs1." + std::to_string(j), ch, ch, k, d, (k * d - d) / 2, true, h3);
          h->res[i][rb][j][1] = B.conv(p + ".convs2." + std::to_string(j), ch, ch, k, 1, (k - 1) / 2, true, h3);
        }
      }
    }
    HostTensor pw = B.weight(g + "conv_post", {1, ch, c.gen_post_k});
    if (!B.bad()) {
      std::vector<float> pk((size_t)c.gen_post_k * ch);
      for (int i = 0; i < ch; ++i)
        for (int j = 0; j < c.gen_post_k; ++j) pk[(size_t)j * ch + i] = pw.data[(size_t)i * c.gen_post_k + j];
      h->post_w = B.upload(pk);
      auto pb = B.need(g + "conv_post.bias", {1});
      if (pb) h->post_b = pb->data[0];
    }
  }
  if (B.bad()) return fail(h, B.e.code, B.e.msg);
  return DCX_OK;
}


int build_weights(dcx_codec* h, bool dry, int32_t with_generator) {
  Builder B{h, dry};
  return build_all(h, B, with_generator);
}

// One conv for the dcx_conv primitive from the tensors "c.weight" / "c.bias" of h->host
// (the h3 weights too: dcx_conv_set_h3 may switch them on later)
int build_conv(dcx_codec* h, int cin, int cout, int k, int dilation, bool transposed, int stride, ConvW& w) {
  Builder B{h, false};
  w = transposed ? B.convT("c", cin, cout, k, stride, true)
                 : B.conv("c", cin, cout, k, dilation, dilation * (k - 1) / 2, true, true);
  return B.e.code;
}

}  // namespace dcx::host
