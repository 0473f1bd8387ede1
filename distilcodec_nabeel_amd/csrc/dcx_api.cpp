// The C ABI of include/distilcodec_amd.h over the host runtime (dcx_host.h): handles, the stage and
// ragged exports, knobs, range flags, the dcx_conv primitive and the profile exports.
#include "dcx_host.h"
#include "dcx_stream_plan.h"

namespace {

void prof_collect(dcx_codec* h) {
  if (h->pending.empty()) return;
  hipDeviceSynchronize();
  for (auto& r : h->pending) {
    float ms = 0.f;
    hipEventElapsedTime(&ms, h->events[r.ev0], h->events[r.ev1]);
    h->prof_launches[r.id] += 1;
    h->prof_ms[r.id] += ms;
    h->prof_flops[r.id] += r.flops;
    h->prof_bytes[r.id] += r.bytes;
  }
  h->pending.clear();
  h->ev_used = 0;
}

// ---- ragged batches (dcx_tokenize_ragged) ---------------------------------------------------
// The plan table (host ints, uploaded by the caller as is): kPlanHead header words, then five prefix
// arrays of batch + 1 entries (dcx::RaggedSeg).
constexpr int kPlanMagic = 0x52414731, kPlanHead = 8;
enum { PLAN_MAGIC = 0, PLAN_BATCH, PLAN_FRAMES, PLAN_SAMPLES, PLAN_T16, PLAN_T4, PLAN_RUN, PLAN_RW };
constexpr int64_t kRaggedMaxSamples = INT32_MAX, kRaggedMaxFrames = 1 << 20, kRaggedMaxBatch = 1 << 20;
int64_t plan_words(int64_t batch) { return kPlanHead + 5 * (batch + 1); }

// The segment descriptor of a plan: totals from the host copy, prefix arrays in the device copy.
bool seg_from_plan(const int32_t* host, const int32_t* dev, int64_t batch, int64_t samples, int64_t frames,
                   dcx::RaggedSeg& g) {
  if (host[PLAN_MAGIC] != kPlanMagic || host[PLAN_BATCH] != batch || host[PLAN_FRAMES] != frames ||
      host[PLAN_SAMPLES] != samples || batch < 1 || batch > kRaggedMaxBatch || frames < batch ||
      frames > kRaggedMaxFrames)
    return false;
  const int64_t n = batch + 1;
  const int32_t* a = dev + kPlanHead;
  g.cu_samples = a;
  g.cu_frames = a + n;
  g.cu_t16 = a + 2 * n;
  g.cu_t4 = a + 3 * n;
  g.cu_run = a + 4 * n;
  g.batch = (int)batch;
  g.rows = (int)frames;
  g.n_t16 = host[PLAN_T16];
  g.n_t4 = host[PLAN_T4];
  g.n_run = host[PLAN_RUN];
  g.rw = host[PLAN_RW];
  // the work-item counts must be the ones the prefix arrays end with (the kernels' grids)
  return g.rw == dcx::dwconv_run_rows(frames) && g.n_t16 >= batch && g.n_t16 <= frames && g.n_t4 >= g.n_t16 &&
         g.n_t4 <= frames && g.n_run >= batch && g.n_run <= frames;
}

// The slot form of the descriptor (dcx_tokenize_slots): batch slots of slot_samples samples in the padded
// layout, the work-item counts those of batch equal clips of that length (dcx_ragged_plan's arithmetic).
// false: a geometry beyond what the kernels index (dcx_ragged_plan's limits).
bool seg_from_slots(const dcx_codec* h, int64_t batch, int64_t slot_samples, const int32_t* n_dev, dcx::RaggedSeg& g) {
  const dcx_config& c = h->cfg;
  const int64_t pad = (c.win - c.hop) / 2, padr = (c.win - c.hop + 1) / 2;
  if (batch < 1 || batch > kRaggedMaxBatch || slot_samples < pad || slot_samples > kRaggedMaxSamples / batch) return false;
  const int64_t wf = frames_of(c, slot_samples + 1);
  if (wf < 1 || wf > kRaggedMaxFrames / batch) return false;
  g = dcx::RaggedSeg{};
  g.batch = (int)batch;
  g.rows = (int)(batch * wf);
  g.rw = dcx::dwconv_run_rows(g.rows);
  g.n_t16 = (int)(batch * ((wf + 15) / 16));
  g.n_t4 = (int)(batch * ((wf + 3) / 4));
  g.n_run = (int)(batch * ((wf + g.rw - 1) / g.rw));
  g.n_dev = n_dev;
  g.slot_samples = (int)slot_samples;
  g.slot_frames = (int)wf;
  g.fr_extra = (int)(pad + padr + 1);
  g.fr_nfft = c.n_fft;
  g.fr_hop = c.hop;
  g.fr_min = (int)pad;
  return true;
}

// what both slot entries refuse before their first launch
int slots_pre(dcx_codec* h, const char* who) {
  if (h->gemm_mode == DCX_GEMM_F32)
    return fail(h, DCX_ERR_INVALID_ARG, std::string(who) + " runs in DCX_GEMM_X6 or DCX_GEMM_BF16 (the intermediates are planes)");
  if (h->split_k >= 2)
    return fail(h, DCX_ERR_STATE, std::string(who) + " with split-K on: the partial sums share one scratch region");
  return DCX_OK;
}

int check_ready(dcx_codec* h, bool need_gen) {
  if (!h) return DCX_ERR_INVALID_ARG;
  if (!h->finalized) return fail(h, DCX_ERR_STATE, "dcx_finalize has not been called");
  if (need_gen && !h->has_gen) return fail(h, DCX_ERR_STATE, "generator weights were not finalized");
  int dev = -1;
  hipGetDevice(&dev);
  if (dev != h->device) return fail(h, DCX_ERR_STATE, "handle belongs to another HIP device");
  return DCX_OK;
}

// a clip of n samples covers the reflect pad and one STFT frame
int check_clip(dcx_codec* h, int64_t n) {
  if (n <= (h->cfg.win - h->cfg.hop) / 2 || frames_of(h->cfg, n) < 1)
    return fail(h, DCX_ERR_INVALID_ARG, "clip too short for the reflect pad / one STFT frame");
  return DCX_OK;
}

}  // namespace

// =========================================================================================
// C ABI
// =========================================================================================
extern "C" {

int dcx_abi_version(void) { return DCX_ABI_VERSION; }

#ifndef DCX_BUILD_ID
#define DCX_BUILD_ID "unversioned"
#endif
const char* dcx_build_id(void) { return DCX_BUILD_ID; }

const char* dcx_status_string(int st) {
  switch (st) {
    case DCX_OK: return "ok";
    case DCX_ERR_INVALID_ARG: return "invalid argument";
    case DCX_ERR_MISSING_WEIGHT: return "missing weight";
    case DCX_ERR_STATE: return "invalid state";
    case DCX_ERR_HIP: return "HIP error";
    case DCX_ERR_OOM: return "out of device memory";
    case DCX_ERR_WORKSPACE: return "workspace too small";
    case DCX_ERR_UNSUPPORTED: return "unsupported input format";
    default: return "unknown status";
  }
}

void dcx_default_config(dcx_config* c) {
  std::memset(c, 0, sizeof(*c));
  c->sample_rate = 24000;
  c->n_fft = 1024; c->hop = 256; c->win = 1024; c->n_mels = 128;
  c->f_min = 0.f; c->f_max = 12000.f;
  const int dep[4] = {3, 3, 9, 3}, dim[4] = {256, 512, 768, 1024};
  for (int i = 0; i < 4; ++i) { c->enc_depths[i] = dep[i]; c->enc_dims[i] = dim[i]; }
  c->vq_dim = 1024; c->codebook_dim = 3584; c->codebook_size = 32768;
  c->gen_channels = 1024; c->gen_pre_k = 13; c->gen_post_k = 13;
  c->n_ups = 5;
  const int ur[5] = {8, 4, 2, 2, 2}, uk[5] = {16, 12, 4, 4, 4};
  for (int i = 0; i < 5; ++i) { c->up_rates[i] = ur[i]; c->up_kernels[i] = uk[i]; }
  c->n_res = 3;
  const int rk[3] = {3, 7, 11};
  for (int i = 0; i < 3; ++i) {
    c->res_kernels[i] = rk[i];
    c->res_dilations[i][0] = 1; c->res_dilations[i][1] = 3; c->res_dilations[i][2] = 5;
  }
}

const char* dcx_last_error(const dcx_codec* h) { return h ? h->err.c_str() : "null handle"; }

int dcx_create(const dcx_config* cfg, dcx_codec** out) {
  if (!cfg || !out) return DCX_ERR_INVALID_ARG;
  *out = nullptr;
  const dcx_config& c = *cfg;
  bool ok = c.n_fft == 1024 && c.win == 1024 && c.hop == 256 && c.n_mels % 16 == 0 && c.n_mels > 0 &&
            c.vq_dim == c.enc_dims[3] && c.codebook_dim % 16 == 0 && c.codebook_size % 128 == 0 &&
            c.n_ups >= 1 && c.n_ups <= 8 && c.n_res == 3 && c.gen_pre_k % 2 == 1 && c.gen_post_k % 2 == 1;
  for (int i = 0; i < 4 && ok; ++i) ok = c.enc_dims[i] % 256 == 0 && c.enc_dims[i] <= 1024 && c.enc_depths[i] >= 0;
  int ch = c.gen_channels;
  for (int i = 0; i < c.n_ups && ok; ++i) {
    ok = c.up_rates[i] >= 1 && c.up_rates[i] <= dcx::kMaxPhases && c.up_kernels[i] % c.up_rates[i] == 0 &&
         (c.up_kernels[i] - c.up_rates[i]) % 2 == 0;
    ch /= 2;
    ok = ok && ch % 32 == 0;
  }
  ok = ok && (ch == 32 || ch == 64);
  for (int i = 0; i < 3 && ok; ++i) ok = c.res_kernels[i] % 2 == 1;
  if (!ok) return DCX_ERR_INVALID_ARG;
  auto h = new (std::nothrow) dcx_codec();
  if (!h) return DCX_ERR_OOM;
  h->cfg = c;
  hipGetDevice(&h->device);
  const char* nrp = std::getenv("DCX_NO_RESPAIR");
  h->res_pair = !(nrp && nrp[0] == '1');
  const char* ncp = std::getenv("DCX_NO_COMPACT");
  h->compact = !(ncp && ncp[0] == '1');
  const char* vpr = std::getenv("DCX_VQ_PAIRS_PER_ROW");
  if (vpr && vpr[0]) h->vq_pairs_per_row = std::max(0, std::atoi(vpr));
  knobs_from_env(h->knobs);
  *out = h;
  return DCX_OK;
}

void dcx_destroy(dcx_codec* h) {
  if (!h) return;
  for (void* p : h->allocs) hipFree(p);
  for (auto e : h->events) hipEventDestroy(e);
  if (h->fork_ev) hipEventDestroy(h->fork_ev);
  if (h->join_ev) hipEventDestroy(h->join_ev);
  if (h->side) hipStreamDestroy(h->side);
  delete h;
}

int dcx_set_tensor(dcx_codec* h, const char* name, const float* data, int32_t ndim, const int64_t* shape) {
  if (!h || !name || (!data && ndim > 0) || ndim < 0 || ndim > 8) return fail(h, DCX_ERR_INVALID_ARG, "bad tensor");
  if (h->finalized) return fail(h, DCX_ERR_STATE, "dcx_set_tensor after dcx_finalize");
  HostTensor t;
  t.shape.assign(shape, shape + ndim);
  const int64_t n = t.numel();
  if (n < 0) return fail(h, DCX_ERR_INVALID_ARG, "negative shape");
  t.data.assign(data, data + n);
  h->host[name] = std::move(t);
  return DCX_OK;
}

int dcx_finalize(dcx_codec* h, int32_t with_generator) {
  if (!h) return DCX_ERR_INVALID_ARG;
  if (h->finalized) return fail(h, DCX_ERR_STATE, "already finalized");
  int rc = build_weights(h, /*dry=*/true, with_generator);  // every required tensor present with the right size, before any upload
  if (rc != DCX_OK) return rc;
  rc = build_weights(h, /*dry=*/false, with_generator);
  if (rc != DCX_OK) return rc;
  h->has_gen = with_generator != 0;
  if (hipStreamCreateWithFlags(&h->side, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreateWithFlags(&h->fork_ev, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&h->join_ev, hipEventDisableTiming) != hipSuccess)
    return fail(h, DCX_ERR_HIP, "dcx_finalize: stream / event creation failed");
  h->finalized = true;
  h->host.clear();
  return DCX_OK;
}

int dcx_set_num_codebooks(dcx_codec* h, int32_t n) {
  if (!h) return DCX_ERR_INVALID_ARG;
  if (h->finalized) return fail(h, DCX_ERR_STATE, "dcx_set_num_codebooks after dcx_finalize");
  if (n < 1 || n > DCX_MAX_CODEBOOKS)
    return fail(h, DCX_ERR_INVALID_ARG, "n_codebooks must be in [1, " + std::to_string(DCX_MAX_CODEBOOKS) + "]");
  h->n_layers = n;
  return DCX_OK;
}

int32_t dcx_num_codebooks(const dcx_codec* h) { return h ? h->n_layers : 0; }

int64_t dcx_num_frames(const dcx_codec* h, int64_t n) { return h ? frames_of(h->cfg, n) : 0; }

size_t dcx_workspace_size(const dcx_codec* h, int32_t batch, int64_t frames) {
  if (!h || batch <= 0 || frames <= 0) return 0;
  dcx_codec* hh = const_cast<dcx_codec*>(h);
  const int64_t n = (frames - 1) * h->cfg.hop + h->cfg.n_fft - (h->cfg.win - h->cfg.hop);
  Bump d(nullptr, 0, true);
  stage_encode_decode(hh, nullptr, batch, n, nullptr, nullptr, d, 0);
  size_t need = d.off;
  Bump q(nullptr, 0, true);  // vq_encode with every optional output in the workspace
  stage_vq_encode(hh, CAct(), batch, (int)frames, nullptr, nullptr, nullptr, nullptr, q, 0);
  need = std::max(need, q.off + (size_t)batch * frames * (h->cfg.codebook_dim + h->cfg.vq_dim) * 4 + 1024);
  if (h->split_k > 1) need += kSplitScratch + 256;  // split-K partial sums (STAGE_PRE)
  return need + 4096;
}

// One stage call on a handle.  A handle is not re-entrant (the header's contract): a second call
// entering while one runs (another thread sharing the handle) is refused with DCX_ERR_STATE rather
// than left to overwrite the first call's split-K scratch pointer.  split_buf is cleared on exit, so
// no later call (or dcx_workspace_size's dry run) sees a pointer into another call's workspace.
struct CallScope {
  dcx_codec* h;
  bool owner = false;
  explicit CallScope(dcx_codec* hh) : h(hh) {
    int expect = 0;
    owner = h && h->busy.compare_exchange_strong(expect, 1);
  }
  ~CallScope() {
    if (owner) {
      h->split_buf = nullptr;
      h->busy.store(0);
    }
  }
};

#define STAGE_PRE(need_gen)                                           \
  int rc_ = check_ready(h, need_gen);                                 \
  if (rc_ != DCX_OK) return rc_;                                      \
  if (batch <= 0) return fail(h, DCX_ERR_INVALID_ARG, "batch must be > 0"); \
  CallScope scope_(h);                                                \
  if (!scope_.owner) return fail(h, DCX_ERR_STATE, "handle in use by a concurrent call (serialise calls per handle)"); \
  hipStream_t s = (hipStream_t)stream;                                \
  Bump ws(workspace, ws_bytes, false);                                \
  h->split_buf = h->split_k > 1 ? (float*)ws.raw(kSplitScratch) : nullptr

int dcx_mel(dcx_codec* h, const float* audio, int32_t batch, int64_t n, float* mel, void* workspace, size_t ws_bytes,
            void* stream) {
  STAGE_PRE(false);
  if (!audio || !mel) return fail(h, DCX_ERR_INVALID_ARG, "null buffer");
  RUN(check_clip(h, n));
  return stage_mel(h, audio, batch, n, Act{mel, nullptr}, ws, s);
}

int dcx_mel_linear(dcx_codec* h, const float* audio, int32_t batch, int64_t n, float* mel, float* log_linear,
                   void* workspace, size_t ws_bytes, void* stream) {
  STAGE_PRE(false);
  if (!audio || !mel || !log_linear) return fail(h, DCX_ERR_INVALID_ARG, "null buffer");
  RUN(check_clip(h, n));
  return stage_mel(h, audio, batch, n, Act{mel, nullptr}, ws, s, log_linear);
}

int dcx_encode(dcx_codec* h, const float* mel, int32_t batch, int64_t frames, float* feat, void* workspace,
               size_t ws_bytes, void* stream) {
  STAGE_PRE(false);
  if (!mel || !feat || frames <= 0) return fail(h, DCX_ERR_INVALID_ARG, "bad arguments");
  return stage_encode(h, CAct(mel, nullptr), batch, (int)frames, Act{feat, nullptr}, ws, s);
}

int dcx_vq_encode(dcx_codec* h, const float* feat, int32_t batch, int64_t frames, int32_t* codes, float* x_pjt_in,
                  float* quantized_fup, float* quantized, void* workspace, size_t ws_bytes, void* stream) {
  STAGE_PRE(false);
  if (!feat || !codes || frames <= 0) return fail(h, DCX_ERR_INVALID_ARG, "bad arguments");
  return stage_vq_encode(h, CAct(feat, nullptr), batch, (int)frames, codes, x_pjt_in, quantized_fup, quantized, ws, s);
}

int dcx_vq_decode(dcx_codec* h, const int32_t* codes, int32_t batch, int64_t frames, float* z, int32_t* n_invalid,
                  void* workspace, size_t ws_bytes, void* stream) {
  STAGE_PRE(false);
  if (!codes || !z || frames <= 0) return fail(h, DCX_ERR_INVALID_ARG, "bad arguments");
  return stage_vq_decode(h, codes, batch, (int)frames, Act{z, nullptr}, n_invalid, ws, s);
}

int dcx_generate(dcx_codec* h, const float* z, int32_t batch, int64_t frames, float* wav, void* workspace,
                 size_t ws_bytes, void* stream) {
  STAGE_PRE(true);
  if (!z || !wav || frames <= 0) return fail(h, DCX_ERR_INVALID_ARG, "bad arguments");
  return stage_generate(h, CAct(z, nullptr), batch, (int)frames, wav, ws, s);
}

int dcx_encode_decode(dcx_codec* h, const float* audio, int32_t batch, int64_t n, int32_t* codes, float* wav,
                      void* workspace, size_t ws_bytes, void* stream) {
  STAGE_PRE(true);
  if (!audio || !codes || !wav) return fail(h, DCX_ERR_INVALID_ARG, "null buffer");
  RUN(check_clip(h, n));
  return stage_encode_decode(h, audio, batch, n, codes, wav, ws, s);
}

int64_t dcx_ragged_plan_size(int32_t batch) { return batch < 1 ? 0 : plan_words(batch); }

int dcx_ragged_plan(dcx_codec* h, const int64_t* clip_samples, int32_t batch, int32_t* plan, int64_t n_words,
                    int64_t* total_samples, int64_t* total_frames) {
  if (!h) return DCX_ERR_INVALID_ARG;
  if (batch < 1 || batch > kRaggedMaxBatch) return fail(h, DCX_ERR_INVALID_ARG, "ragged plan: batch must be in [1, 2^20]");
  if (!clip_samples || !plan) return fail(h, DCX_ERR_INVALID_ARG, "ragged plan: null buffer");
  if (n_words < plan_words(batch))
    return fail(h, DCX_ERR_INVALID_ARG, "ragged plan: the table holds " + std::to_string(n_words) + " words, " +
                                            std::to_string(plan_words(batch)) + " needed (dcx_ragged_plan_size)");
  const int64_t pad = (h->cfg.win - h->cfg.hop) / 2;
  const int64_t n = (int64_t)batch + 1;
  int32_t *cs = plan + kPlanHead, *cf = cs + n, *c16 = cf + n, *c4 = c16 + n, *cr = c4 + n;
  // pass 1: the totals (the run length follows from the total row count)
  int64_t samples = 0, frames = 0;
  for (int32_t b = 0; b < batch; ++b) {
    const int64_t nb = clip_samples[b];
    if (nb < pad)
      return fail(h, DCX_ERR_INVALID_ARG, "ragged plan: clip " + std::to_string(b) + " has " + std::to_string(nb) +
                                              " samples, fewer than the reflect pad's " + std::to_string(pad));
    if (nb > kRaggedMaxSamples - samples)
      return fail(h, DCX_ERR_INVALID_ARG, "ragged plan: more than 2^31 - 1 samples in all (at clip " + std::to_string(b) + ")");
    samples += nb;
    frames += frames_of(h->cfg, nb + 1);
    if (frames > kRaggedMaxFrames)
      return fail(h, DCX_ERR_INVALID_ARG, "ragged plan: more than 2^20 frames in all (at clip " + std::to_string(b) + ")");
  }
  const int rw = dcx::dwconv_run_rows(frames);
  cs[0] = cf[0] = c16[0] = c4[0] = cr[0] = 0;
  for (int32_t b = 0; b < batch; ++b) {
    const int64_t T = frames_of(h->cfg, clip_samples[b] + 1);
    cs[b + 1] = (int32_t)(cs[b] + clip_samples[b]);
    cf[b + 1] = (int32_t)(cf[b] + T);
    c16[b + 1] = (int32_t)(c16[b] + (T + 15) / 16);
    c4[b + 1] = (int32_t)(c4[b] + (T + 3) / 4);
    cr[b + 1] = (int32_t)(cr[b] + (T + rw - 1) / rw);
  }
  plan[PLAN_MAGIC] = kPlanMagic;
  plan[PLAN_BATCH] = batch;
  plan[PLAN_FRAMES] = (int32_t)frames;
  plan[PLAN_SAMPLES] = (int32_t)samples;
  plan[PLAN_T16] = c16[batch];
  plan[PLAN_T4] = c4[batch];
  plan[PLAN_RUN] = cr[batch];
  plan[PLAN_RW] = rw;
  if (total_samples) *total_samples = samples;
  if (total_frames) *total_frames = frames;
  return DCX_OK;
}

size_t dcx_ragged_workspace_size(const dcx_codec* h, int32_t batch, int64_t total_frames) {
  if (!h || batch < 1 || total_frames < batch || total_frames > kRaggedMaxFrames) return 0;
  dcx::RaggedSeg g{};
  g.batch = batch;
  g.rows = (int)total_frames;
  Bump d(nullptr, 0, true);
  tokenize_ragged_rows(const_cast<dcx_codec*>(h), nullptr, g, nullptr, nullptr, nullptr, d, 0);
  return d.off + 4096;
}

int dcx_tokenize_ragged(dcx_codec* h, const float* audio_packed, const int32_t* plan_dev, const int32_t* plan_host,
                        int32_t batch, int64_t total_samples, int64_t total_frames, int32_t* codes, float* x_pjt_in,
                        float* quantized_fup, void* workspace, size_t ws_bytes, void* stream) {
  STAGE_PRE(false);
  if (!audio_packed || !plan_dev || !plan_host || !codes) return fail(h, DCX_ERR_INVALID_ARG, "null buffer");
  if (h->gemm_mode == DCX_GEMM_F32)
    return fail(h, DCX_ERR_INVALID_ARG, "dcx_tokenize_ragged runs in DCX_GEMM_X6 or DCX_GEMM_BF16 (the packed tensors are planes)");
  if (h->split_k >= 2)
    return fail(h, DCX_ERR_STATE, "dcx_tokenize_ragged with split-K on: the partial sums share one scratch region");
  dcx::RaggedSeg g{};
  if (!seg_from_plan(plan_host, plan_dev, batch, total_samples, total_frames, g))
    return fail(h, DCX_ERR_INVALID_ARG, "ragged plan does not match batch / total_samples / total_frames (dcx_ragged_plan)");
  return tokenize_ragged_rows(h, audio_packed, g, codes, x_pjt_in, quantized_fup, ws, s);
}

// the call's workspace need, checked before the first launch (a later stage's shortage would otherwise
// be found after earlier stages have run)
static int slots_workspace(dcx_codec* h, const dcx::RaggedSeg& g, size_t ws_bytes, const char* who) {
  Bump dry(nullptr, 0, true);
  RUN(tokenize_slots_rows(h, nullptr, g, nullptr, nullptr, dry, 0));
  if (ws_bytes < dry.off)
    return fail(h, DCX_ERR_WORKSPACE, std::string(who) + ": workspace too small (dcx_ragged_workspace_size(h, batch, batch * slot frames))");
  return DCX_OK;
}

int dcx_tokenize_slots(dcx_codec* h, const float* audio, const int32_t* n_samples_dev, int32_t batch,
                       int64_t slot_samples, int32_t* codes, float* x_pjt_in, void* workspace, size_t ws_bytes,
                       void* stream) {
  STAGE_PRE(false);
  if (!audio || !n_samples_dev || !codes) return fail(h, DCX_ERR_INVALID_ARG, "null buffer");
  RUN(slots_pre(h, "dcx_tokenize_slots"));
  dcx::RaggedSeg g{};
  if (!seg_from_slots(h, batch, slot_samples, n_samples_dev, g))
    return fail(h, DCX_ERR_INVALID_ARG, "dcx_tokenize_slots: slot_samples below the reflect pad's 384, or more than 2^31 - 1 samples / 2^20 frames in all");
  RUN(slots_workspace(h, g, ws_bytes, "dcx_tokenize_slots"));
  return tokenize_slots_rows(h, audio, g, codes, x_pjt_in, ws, s);
}

// Ragged decode: the padded layout with per-clip lengths in device memory.  The checks
// both entries share; the kernels' own limits are checked where they are launched (stage_generate).
static int ragged_decode_pre(dcx_codec* h, const void* in, const int32_t* lengths_dev, int64_t frames_max,
                             const float* wav) {
  if (!in || !lengths_dev || !wav || frames_max <= 0 || frames_max > INT32_MAX / 256)
    return fail(h, DCX_ERR_INVALID_ARG, "ragged decode: null buffer or bad frames_max");
  if (h->split_k >= 2)
    return fail(h, DCX_ERR_STATE, "ragged decode with split-K on: the split kernels' reduce is not length-aware");
  if (h->gemm_mode != DCX_GEMM_X6)
    return fail(h, DCX_ERR_INVALID_ARG, "ragged decode runs in DCX_GEMM_X6 (the other modes' kernels are not length-aware)");
  return DCX_OK;
}

int dcx_generate_ragged(dcx_codec* h, const float* z, const int32_t* lengths_dev, int32_t batch, int64_t frames_max,
                        float* wav, void* workspace, size_t ws_bytes, void* stream) {
  if (h && (!z || !lengths_dev)) return fail(h, DCX_ERR_INVALID_ARG, "ragged decode: null buffer");
  STAGE_PRE(true);
  RUN(ragged_decode_pre(h, z, lengths_dev, frames_max, wav));
  return stage_generate(h, CAct(z, nullptr), batch, (int)frames_max, wav, ws, s, lengths_dev);
}

int dcx_decode_ragged(dcx_codec* h, const int32_t* codes, const int32_t* lengths_dev, int32_t batch,
                      int64_t frames_max, float* wav, int32_t* n_invalid, void* workspace, size_t ws_bytes,
                      void* stream) {
  if (h && (!codes || !lengths_dev)) return fail(h, DCX_ERR_INVALID_ARG, "ragged decode: null buffer");
  STAGE_PRE(true);
  RUN(ragged_decode_pre(h, codes, lengths_dev, frames_max, wav));
  return stage_decode_ragged(h, codes, lengths_dev, batch, (int)frames_max, wav, n_invalid, ws, s);
}

// Token streams: the geometry every entry takes, and the views of the caller's state
// buffer for it (false: refused, with the reason in dcx_last_error).
static bool stream_geometry(const dcx_codec* h, int32_t sessions, int32_t push, int32_t halo) {
  return h && sessions >= 1 && sessions <= dcx::kStreamMaxSessions && push >= 1 && push <= dcx::kStreamMaxFrames &&
         halo >= 0 && halo <= dcx::kStreamMaxFrames;
}

static int stream_state(dcx_codec* h, void* state, size_t state_bytes, int32_t sessions, int32_t push, int32_t halo,
                        dcx::StreamState& st) {
  if (!stream_geometry(h, sessions, push, halo))
    return fail(h, DCX_ERR_INVALID_ARG, "token stream: sessions must be in [1, 65535], push_frames in [1, 65536], halo_frames in [0, 65536]");
  if (!state || (reinterpret_cast<uintptr_t>(state) & 15))
    return fail(h, DCX_ERR_INVALID_ARG, "token stream: null or misaligned state buffer (16 bytes)");
  const size_t need = dcx::stream_state_layout(state, sessions, push, halo, h->n_layers, h->cfg.hop, st);
  if (state_bytes < need)
    return fail(h, DCX_ERR_INVALID_ARG, "token stream: the state buffer holds " + std::to_string(state_bytes) + " bytes, " +
                                            std::to_string(need) + " needed (dcx_stream_state_size)");
  return DCX_OK;
}

size_t dcx_stream_state_size(const dcx_codec* h, int32_t sessions, int32_t push_frames, int32_t halo_frames) {
  if (!stream_geometry(h, sessions, push_frames, halo_frames)) return 0;
  dcx::StreamState st{};
  return dcx::stream_state_layout(nullptr, sessions, push_frames, halo_frames, h->n_layers, h->cfg.hop, st);
}

int dcx_stream_plan_step(int32_t halo_frames, int32_t push_frames, int32_t* T, int32_t* E, int32_t* closed, int32_t n_new,
                         int32_t flags, int32_t* len, int32_t* skip, int32_t* take) {
  if (halo_frames < 0 || push_frames < 1 || !T || !E || !closed) return DCX_ERR_INVALID_ARG;
  dcx::StreamSlot s{*T, *E, *closed};
  const dcx::StreamStep o = dcx::stream_plan_step(halo_frames, push_frames, s, n_new, flags);
  *T = s.T;
  *E = s.E;
  *closed = s.closed;
  if (len) *len = o.len;
  if (skip) *skip = o.skip;
  if (take) *take = o.take;
  return DCX_OK;
}

int dcx_stream_reset(dcx_codec* h, void* state, size_t state_bytes, int32_t sessions, int32_t push_frames,
                     int32_t halo_frames, void* stream) {
  if (!h) return DCX_ERR_INVALID_ARG;
  dcx::StreamState st{};
  RUN(stream_state(h, state, state_bytes, sessions, push_frames, halo_frames, st));
  RUN(check_ready(h, false));
  HIPCHK(h, dcx::launch_stream_reset(st, (hipStream_t)stream));
  return DCX_OK;
}

int dcx_stream_decode_step(dcx_codec* h, void* state, size_t state_bytes, int32_t sessions, int32_t push_frames,
                           int32_t halo_frames, const int32_t* new_codes, const int32_t* n_new_dev,
                           const int32_t* flags_dev, float* wav_out, int32_t* n_out_dev, int32_t* n_invalid,
                           void* workspace, size_t ws_bytes, void* stream) {
  if (!h) return DCX_ERR_INVALID_ARG;
  dcx::StreamState st{};
  RUN(stream_state(h, state, state_bytes, sessions, push_frames, halo_frames, st));
  if (!new_codes || !n_new_dev || !flags_dev || !wav_out || !n_out_dev || (reinterpret_cast<uintptr_t>(wav_out) & 15))
    return fail(h, DCX_ERR_INVALID_ARG, "token stream: null buffer, or wav_out not on a 16-byte boundary");
  const int32_t batch = sessions;
  STAGE_PRE(true);
  RUN(ragged_decode_pre(h, new_codes, st.len, st.W, wav_out));
  // what the decode would refuse after the plan kernel has run is refused here, before any launch
  Bump dry(nullptr, 0, true);
  RUN(stage_decode_ragged(h, nullptr, nullptr, batch, st.W, nullptr, nullptr, dry, s));
  if (ws_bytes < dry.off)
    return fail(h, DCX_ERR_INVALID_ARG, "token stream: workspace too small (dcx_workspace_size(h, sessions, push_frames + 2 halo_frames))");
  return stage_stream_step(h, st, new_codes, n_new_dev, flags_dev, wav_out, n_out_dev, n_invalid, ws, s);
}

// Audio streams: the geometry every entry takes, the views of the caller's state buffer
// and the slot descriptor of the step's tokenization (its lengths: the plan kernel's len array).
static dcx::AudioGeom audio_geom(const dcx_codec* h) {
  const dcx_config& c = h->cfg;
  return dcx::AudioGeom{c.hop, c.n_fft, (c.win - c.hop) / 2, (c.win - c.hop + 1) / 2};
}

static bool audio_stream_geometry(const dcx_codec* h, int32_t sessions, int32_t push, int32_t halo, dcx::RaggedSeg* g) {
  if (!h || sessions < 1 || sessions > dcx::kStreamMaxSessions || push < 1 || push > dcx::kAudioStreamMaxPush || halo < 0 ||
      halo > dcx::kStreamMaxFrames || h->cfg.hop < 4 || h->cfg.hop % 4 || h->cfg.codebook_dim % 4)
    return false;
  dcx::RaggedSeg tmp{};
  return seg_from_slots(h, sessions, dcx::audio_window_samples(audio_geom(h), halo, push), nullptr, g ? *g : tmp);
}

static int audio_stream_state(dcx_codec* h, void* state, size_t state_bytes, int32_t sessions, int32_t push, int32_t halo,
                              int32_t want_pjt_in, dcx::AudioStreamState& st, dcx::RaggedSeg& g) {
  if (!audio_stream_geometry(h, sessions, push, halo, &g))
    return fail(h, DCX_ERR_INVALID_ARG, "audio stream: sessions must be in [1, 65535], push_samples in [1, 2^24], halo_frames in [0, 65536], and the windows within 2^31 - 1 samples and 2^20 frames in all");
  if (!state || (reinterpret_cast<uintptr_t>(state) & 15))
    return fail(h, DCX_ERR_INVALID_ARG, "audio stream: null or misaligned state buffer (16 bytes)");
  const size_t need = dcx::audio_stream_state_layout(state, sessions, push, halo, h->n_layers,
                                                     want_pjt_in ? h->cfg.codebook_dim : 0, audio_geom(h), st);
  if (state_bytes < need)
    return fail(h, DCX_ERR_INVALID_ARG, "audio stream: the state buffer holds " + std::to_string(state_bytes) + " bytes, " +
                                            std::to_string(need) + " needed (dcx_stream_encode_state_size)");
  g.n_dev = st.len;
  return DCX_OK;
}

size_t dcx_stream_encode_state_size(const dcx_codec* h, int32_t sessions, int32_t push_samples, int32_t halo_frames,
                                    int32_t want_pjt_in) {
  if (!audio_stream_geometry(h, sessions, push_samples, halo_frames, nullptr)) return 0;
  dcx::AudioStreamState st{};
  return dcx::audio_stream_state_layout(nullptr, sessions, push_samples, halo_frames, h->n_layers,
                                        want_pjt_in ? h->cfg.codebook_dim : 0, audio_geom(h), st);
}

int dcx_stream_encode_geometry(const dcx_codec* h, int32_t push_samples, int32_t halo_frames, int64_t* window_samples,
                               int64_t* window_frames, int64_t* out_frames) {
  if (!h || push_samples < 1 || push_samples > dcx::kAudioStreamMaxPush || halo_frames < 0 || halo_frames > dcx::kStreamMaxFrames)
    return DCX_ERR_INVALID_ARG;
  const dcx::AudioGeom g = audio_geom(h);
  const int64_t ws = dcx::audio_window_samples(g, halo_frames, push_samples);
  if (window_samples) *window_samples = ws;
  if (window_frames) *window_frames = ws / g.hop;
  if (out_frames) *out_frames = dcx::audio_take_max(g, halo_frames, push_samples);
  return DCX_OK;
}

int dcx_stream_encode_plan_step(const dcx_codec* h, int32_t halo_frames, int32_t push_samples, int32_t* M, int32_t* C,
                                int32_t* closed, int32_t n_new, int32_t flags, int32_t* len, int32_t* start,
                                int32_t* skip, int32_t* take) {
  if (!h || halo_frames < 0 || push_samples < 1 || !M || !C || !closed) return DCX_ERR_INVALID_ARG;
  dcx::AudioSlot s{*M, *C, *closed};
  const dcx::AudioStep o = dcx::audio_plan_step(audio_geom(h), halo_frames, push_samples, s, n_new, flags);
  *M = s.M;
  *C = s.C;
  *closed = s.closed;
  if (len) *len = o.len;
  if (start) *start = o.start;
  if (skip) *skip = o.skip;
  if (take) *take = o.take;
  return DCX_OK;
}

int dcx_stream_encode_reset(dcx_codec* h, void* state, size_t state_bytes, int32_t sessions, int32_t push_samples,
                            int32_t halo_frames, int32_t want_pjt_in, void* stream) {
  if (!h) return DCX_ERR_INVALID_ARG;
  dcx::AudioStreamState st{};
  dcx::RaggedSeg g{};
  RUN(audio_stream_state(h, state, state_bytes, sessions, push_samples, halo_frames, want_pjt_in, st, g));
  RUN(check_ready(h, false));
  HIPCHK(h, dcx::launch_audio_stream_reset(st, (hipStream_t)stream));
  return DCX_OK;
}

int dcx_stream_encode_step(dcx_codec* h, void* state, size_t state_bytes, int32_t sessions, int32_t push_samples,
                           int32_t halo_frames, const float* new_samples, const int32_t* n_new_dev,
                           const int32_t* flags_dev, int32_t* codes_out, int32_t* n_out_dev, float* x_pjt_in_out,
                           void* workspace, size_t ws_bytes, void* stream) {
  if (!h) return DCX_ERR_INVALID_ARG;
  dcx::AudioStreamState st{};
  dcx::RaggedSeg g{};
  // a state buffer laid out with the x_pjt_in window exactly when the caller takes x_pjt_in
  RUN(audio_stream_state(h, state, state_bytes, sessions, push_samples, halo_frames, x_pjt_in_out ? 1 : 0, st, g));
  if (!new_samples || !n_new_dev || !flags_dev || !codes_out || !n_out_dev ||
      (reinterpret_cast<uintptr_t>(x_pjt_in_out) & 15))
    return fail(h, DCX_ERR_INVALID_ARG, "audio stream: null buffer, or x_pjt_in_out not on a 16-byte boundary");
  const int32_t batch = sessions;
  STAGE_PRE(false);
  // what the tokenization would refuse after the plan kernel has run is refused here, before any launch
  RUN(slots_pre(h, "dcx_stream_encode_step"));
  RUN(slots_workspace(h, g, ws_bytes, "dcx_stream_encode_step"));
  return stage_audio_stream_step(h, st, g, new_samples, n_new_dev, flags_dev, codes_out, n_out_dev, x_pjt_in_out, ws, s);
}

int dcx_module_io(const dcx_codec* h, const char* module, int32_t* in_channels, int32_t* out_channels,
                  int32_t* out_rate) {
  if (!h || !module) return DCX_ERR_INVALID_ARG;
  int ci = 0, co = 0, r = 1;
  // a read-only query: an unknown name returns DCX_ERR_INVALID_ARG without touching the handle's
  // last-error string (another thread may be running a stage call on the handle)
  if (!module_io(h, module, ci, co, r)) return DCX_ERR_INVALID_ARG;
  if (in_channels) *in_channels = ci;
  if (out_channels) *out_channels = co;
  if (out_rate) *out_rate = r;
  return DCX_OK;
}

size_t dcx_module_workspace_size(const dcx_codec* h, const char* module, int32_t batch, int64_t rows) {
  if (!h || !module || batch <= 0 || rows <= 0 || !h->finalized) return 0;
  Bump d(nullptr, 0, true);
  if (stage_module(const_cast<dcx_codec*>(h), module, nullptr, batch, (int)rows, nullptr, d, 0) != DCX_OK) return 0;
  // the split-K partial sums, carved ahead of the module's buffers (STAGE_PRE)
  return d.off + 4096 + (h->split_k > 1 ? kSplitScratch + 256 : 0);
}

int dcx_module_forward(dcx_codec* h, const char* module, const float* x, int32_t batch, int64_t rows,
                       int32_t channels, void* y, void* workspace, size_t ws_bytes, void* stream) {
  STAGE_PRE(false);
  if (!module || !x || !y || rows <= 0 || rows > (1 << 30)) return fail(h, DCX_ERR_INVALID_ARG, "bad arguments");
  int ci = 0, co = 0, r = 1;
  if (!module_io(h, module, ci, co, r)) return fail(h, DCX_ERR_INVALID_ARG, std::string("unknown module: ") + module);
  // the kernels read cin channels per row: any other width would be read out of bounds
  if (channels != ci)
    return fail(h, DCX_ERR_INVALID_ARG, std::string(module) + " takes " + std::to_string(ci) + " input channels, got " +
                                            std::to_string(channels));
  return stage_module(h, module, x, batch, (int)rows, y, ws, s);
}

int dcx_transpose(const float* in, float* out, int32_t batch, int64_t rows, int64_t cols, void* stream) {
  if (!in || !out || batch <= 0 || rows <= 0 || cols <= 0) return DCX_ERR_INVALID_ARG;
  return dcx::launch_transpose(in, out, batch, rows, cols, (hipStream_t)stream) == hipSuccess ? DCX_OK : DCX_ERR_HIP;
}

int dcx_resample_poly(const float* x, int32_t batch, int64_t n_in, int64_t x_stride, const double* h, int32_t h_len,
                      int32_t up, int32_t down, int64_t pre, float* y, int64_t n_out, int64_t y_stride, void* stream) {
  if (!x || !h || !y || batch <= 0 || n_in <= 0 || n_out <= 0 || h_len <= 0 || up <= 0 || down <= 0 || pre < 0 ||
      x_stride < n_in || y_stride < n_out || batch > 65535)
    return DCX_ERR_INVALID_ARG;
  // the largest filter index a thread can form must fit: t - up * m_lo < h_len by construction;
  // t itself must not overflow
  if ((pre + n_out) > (INT64_MAX / down)) return DCX_ERR_INVALID_ARG;
  return dcx::launch_resample_poly(x, batch, n_in, x_stride, h, h_len, up, down, pre, y, n_out, y_stride,
                                   (hipStream_t)stream) == hipSuccess
             ? DCX_OK
             : DCX_ERR_HIP;
}

int dcx_set_gemm_mode(dcx_codec* h, int32_t mode) {
  if (!h) return DCX_ERR_INVALID_ARG;
  if (mode != DCX_GEMM_F32 && mode != DCX_GEMM_X6 && mode != DCX_GEMM_BF16)
    return fail(h, DCX_ERR_INVALID_ARG, "unknown GEMM mode");
  h->gemm_mode = mode;
  return DCX_OK;
}

int32_t dcx_get_gemm_mode(const dcx_codec* h) { return h ? h->gemm_mode : -1; }

int dcx_set_split_k(dcx_codec* h, int32_t max_splits) {
  if (!h || max_splits < 0 || max_splits > kSplitMax) return DCX_ERR_INVALID_ARG;
  h->split_k = max_splits;
  return DCX_OK;
}

int dcx_set_knob(dcx_codec* h, const char* name, int32_t value) {
  if (!h || !name) return DCX_ERR_INVALID_ARG;
  // claim the handle as a stage call does (CallScope), so no call starts while the knob changes
  CallScope scope(h);
  if (!scope.owner) return fail(h, DCX_ERR_STATE, "dcx_set_knob during a stage call");
  const auto k = knob_slot(name);
  if (!k) return fail(h, DCX_ERR_INVALID_ARG, std::string("unknown knob: ") + name);
  h->knobs.*k = value;
  return DCX_OK;
}

int dcx_get_knob(const dcx_codec* h, const char* name, int32_t* value) {
  if (!h || !name || !value) return DCX_ERR_INVALID_ARG;
  const auto k = knob_slot(name);
  if (!k) return DCX_ERR_INVALID_ARG;
  *value = h->knobs.*k;
  return DCX_OK;
}

int dcx_range_flags(dcx_codec* h, int32_t* flags, int32_t reset) {
  if (!h || !flags) return DCX_ERR_INVALID_ARG;
  *flags = 0;
  if (!h->rflag) return DCX_OK;  // not finalized: no h3 call has run
  int v = 0;
  if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(&v, h->rflag, sizeof v, hipMemcpyDeviceToHost) != hipSuccess)
    return fail(h, DCX_ERR_HIP, "reading the range flags failed");
  *flags = v;
  if (reset && hipMemset(h->rflag, 0, sizeof v) != hipSuccess) return fail(h, DCX_ERR_HIP, "resetting the range flags failed");
  return DCX_OK;
}

}  // extern "C"

struct dcx_conv {
  dcx_codec scratch;  // owns the device allocations and the last error
  ConvW w;
  unsigned short* planes = nullptr;  // x6 input planes (or the h2 layout) of the last call (grown on demand)
  size_t planes_cap = 0;
  bool h3 = false;         // dcx_conv_set_h3: h3 arithmetic where the stages would use it
  int* range = nullptr;    // h3: per-clip max |x| [batch], then the clips' or rows' shifts
  size_t range_cap = 0;    // words
};

// A device buffer of the primitive grown to `need` elements (contents not kept); false when out of memory
template <class T>
static bool grow(T*& p, size_t& cap, size_t need) {
  if (need <= cap) return true;
  if (p) hipFree(p);
  p = nullptr;
  cap = 0;
  if (hipMalloc(&p, need * sizeof(T)) != hipSuccess) return false;
  cap = need;
  return true;
}

extern "C" {

int dcx_conv_create(const float* weight, const float* bias, int32_t cin, int32_t cout, int32_t k, int32_t dilation,
                    int32_t transposed, int32_t stride, dcx_conv** out) {
  if (!weight || !out || cin <= 0 || cout <= 0 || k <= 0 || dilation <= 0 || stride <= 0) return DCX_ERR_INVALID_ARG;
  if (cin % 16 || cout % 32) return DCX_ERR_INVALID_ARG;
  if (transposed && (k % stride || (k - stride) % 2 || stride > dcx::kMaxPhases)) return DCX_ERR_INVALID_ARG;
  if (!transposed && (k % 2 == 0)) return DCX_ERR_INVALID_ARG;
  auto c = new (std::nothrow) dcx_conv();
  if (!c) return DCX_ERR_OOM;
  dcx_codec* h = &c->scratch;
  HostTensor wt;
  const int64_t n = (int64_t)cin * cout * k;
  wt.shape = transposed ? std::vector<int64_t>{cin, cout, k} : std::vector<int64_t>{cout, cin, k};
  wt.data.assign(weight, weight + n);
  h->host["c.weight"] = wt;
  HostTensor bt;
  bt.shape = {cout};
  if (bias) bt.data.assign(bias, bias + cout); else bt.data.assign(cout, 0.f);
  h->host["c.bias"] = bt;
  const int code = build_conv(h, cin, cout, k, dilation, transposed != 0, stride, c->w);
  h->host.clear();
  if (code != DCX_OK) {
    dcx_conv_destroy(c);
    return code;
  }
  *out = c;
  return DCX_OK;
}

}  // extern "C"

// The primitive's call: the input in the form its GEMM mode takes, then `outputs(cc, h3)` fills in the
// call's outputs and epilogue (h3: the conv runs in h3 arithmetic, cc.x.r holding the input's range)
template <class Outputs>
static int conv_forward(dcx_conv* c, int32_t gemm_mode, const float* x, int32_t batch, int64_t lin, void* stream,
                        Outputs outputs) {
  dcx_codec* h = &c->scratch;
  h->gemm_mode = gemm_mode;
  hipStream_t s = (hipStream_t)stream;
  CAct xa(x, nullptr);
  bool h3 = false;
  if (gemm_mode != DCX_GEMM_F32 && gemm_mode != DCX_GEMM_X6 && gemm_mode != DCX_GEMM_BF16) return DCX_ERR_INVALID_ARG;
  if (gemm_mode != DCX_GEMM_F32 && !f32_input_ok(c->w)) {
    const size_t need = (size_t)batch * lin * c->w.cin * 3;
    if (!grow(c->planes, c->planes_cap, need)) return DCX_ERR_OOM;
    // h3 (dcx_conv_set_h3): the input in the h2 layout, range-scaled as ensure_planes does for a
    // caller's tensor: per clip (exact max) for the tap convs, per row for a one-tap Conv1d
    h3 = c->h3 && (c->w.taps >= 2 ? takes_h3_conv(h, c->w, lin) : takes_h3(h, c->w));
    if (h3) {
      const long long rows = (long long)batch * lin;
      const size_t words = (size_t)batch + (size_t)std::max<long long>(batch, rows);
      if (!grow(c->range, c->range_cap, words)) return DCX_ERR_OOM;
      float* am = reinterpret_cast<float*>(c->range);
      int* ash = c->range + batch;
      xa.r = Rng{};
      if (c->w.taps >= 2) {
        if (dcx::launch_h2_ranged(x, nullptr, c->planes, batch, lin, c->w.cin, 0, 0.f, am, ash, h->rflag, s) != hipSuccess)
          return fail(h, DCX_ERR_HIP, "h3 input split (per clip) failed");
        xa.r.ash = ash;
        xa.r.amax = am;
      } else {
        if (dcx::launch_h2_rows(x, c->planes, rows, c->w.cin, ash, s) != hipSuccess)
          return fail(h, DCX_ERR_HIP, "h3 input split (per row) failed: Cin must be 256, 512, 768, 1024 or a multiple of 32 below 256");
        xa.r.ash_row = ash;
      }
      xa.lay = dcx::LAYOUT_H2;
    } else if (dcx::launch_split_planes(x, c->planes, (long long)batch * lin, c->w.cin, dcx::LAYOUT_PLANES, s) != hipSuccess) {
      return DCX_ERR_HIP;
    }
    xa.p = c->planes;
  }
  ConvCall cc = framed(xa, batch, (int)lin, c->w.cin);
  const int code = outputs(cc, h3);
  return code != DCX_OK ? code : run_conv(h, c->w, cc, s);
}

extern "C" {

int dcx_conv_forward(dcx_conv* c, int32_t gemm_mode, const float* x, int32_t batch, int64_t lin, float* y,
                     float* y_silu, const float* res, int32_t epi, void* stream) {
  if (!c || !x || batch <= 0 || lin <= 0 || (!y && !y_silu)) return DCX_ERR_INVALID_ARG;
  if (epi != dcx::EPI_BIAS && epi != dcx::EPI_GELU && epi != dcx::EPI_RES) return DCX_ERR_INVALID_ARG;
  if (epi == dcx::EPI_RES && !res) return DCX_ERR_INVALID_ARG;
  return conv_forward(c, gemm_mode, x, batch, lin, stream, [&](ConvCall& cc, bool) -> int {
    cc.y = y;
    cc.y2 = y_silu;
    cc.res = res;
    cc.epi = epi;
    return DCX_OK;
  });
}

int dcx_conv_forward_h3(dcx_conv* c, const float* x, int32_t batch, int64_t lin, const dcx_conv_h3_out* o, void* stream) {
  if (!c || !x || !o || batch <= 0 || lin <= 0 || c->w.taps < 2 || c->w.phases != 1) return DCX_ERR_INVALID_ARG;
  if (o->epi != dcx::EPI_BIAS && o->epi != dcx::EPI_RES) return DCX_ERR_INVALID_ARG;
  if (o->mean < dcx::MEAN_NONE || o->mean > dcx::MEAN_LAST || (o->mean != dcx::MEAN_NONE && !o->macc)) return DCX_ERR_INVALID_ARG;
  if (o->epi == dcx::EPI_RES && (!o->res || !o->res_amax)) return DCX_ERR_INVALID_ARG;
  if (o->mean >= dcx::MEAN_MID && !o->macc_amax) return DCX_ERR_INVALID_ARG;
  if (o->y_silu_h2 && !o->y_ash) return DCX_ERR_INVALID_ARG;
  return conv_forward(c, DCX_GEMM_X6, x, batch, lin, stream, [&](ConvCall& cc, bool h3) -> int {
    if (!h3) return fail(&c->scratch, DCX_ERR_INVALID_ARG, "dcx_conv_forward_h3: not an h3 conv (dcx_conv_set_h3, Cout % 128)");
    cc.y = o->y;
    cc.y2 = o->y_silu;
    cc.y6s = o->y_silu_h2;
    cc.ys_lay = dcx::LAYOUT_H2;
    cc.res = o->res;
    cc.macc = o->macc;
    cc.epi = o->epi;
    cc.mean = o->mean;
    // |v| <= g max|x| + max|b| (+ max|res|, + max|macc|: the mean's third is left out, a looser bound)
    cc.yb = prog_conv(c->w, cc.x.r);
    if (o->res) prog_add(cc.yb, 1.0f, Rng{nullptr, 0, o->res_amax, 0.f});
    if (o->mean >= dcx::MEAN_MID) prog_add(cc.yb, 1.0f, Rng{nullptr, 0, o->macc_amax, 0.f});
    cc.y_amax = o->y_amax;
    cc.y_ash = o->y_silu_h2 ? o->y_ash : nullptr;
    cc.ragged(o->lens, (int)lin);
    return DCX_OK;
  });
}

void dcx_conv_destroy(dcx_conv* c) {
  if (!c) return;
  if (c->planes) hipFree(c->planes);
  if (c->range) hipFree(c->range);
  for (void* p : c->scratch.allocs) hipFree(p);
  delete c;
}

const char* dcx_conv_last_kernel(const dcx_conv* c) { return c ? c->scratch.last_kname : ""; }

int dcx_epi_form_launches(int64_t* counts, int32_t n, int32_t reset) {
  if (!counts || n != dcx::kEpiFormCounters) return DCX_ERR_INVALID_ARG;
  long long v[dcx::kEpiFormCounters];
  dcx::epi_form_launches(v, reset != 0);
  for (int i = 0; i < n; ++i) counts[i] = v[i];
  return DCX_OK;
}

int dcx_conv_set_knob(dcx_conv* c, const char* name, int32_t value) {
  if (!c || !name) return DCX_ERR_INVALID_ARG;
  const auto k = knob_slot(name);
  if (!k) return fail(&c->scratch, DCX_ERR_INVALID_ARG, std::string("unknown knob: ") + name);
  c->scratch.knobs.*k = value;
  return DCX_OK;
}

int dcx_conv_set_h3(dcx_conv* c, int32_t on) {
  if (!c) return DCX_ERR_INVALID_ARG;
  c->h3 = on != 0;
  return DCX_OK;
}

int dcx_profile_enable(dcx_codec* h, int32_t on) {
  if (!h) return DCX_ERR_INVALID_ARG;
  h->prof = on != 0;
  return DCX_OK;
}

int dcx_profile_reset(dcx_codec* h) {
  if (!h) return DCX_ERR_INVALID_ARG;
  prof_collect(h);
  for (size_t i = 0; i < h->prof_names.size(); ++i) {
    h->prof_launches[i] = 0;
    h->prof_ms[i] = h->prof_flops[i] = h->prof_bytes[i] = 0;
  }
  return DCX_OK;
}

int dcx_vq_rescore_stats(dcx_codec* h, int64_t* rows_rescored, int64_t* codes_rescored, int32_t reset) {
  if (!h || !h->vq_stats) return DCX_ERR_STATE;
  h->vq_stats_on = true;
  int v[2] = {0, 0};
  if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(v, h->vq_stats, sizeof v, hipMemcpyDeviceToHost) != hipSuccess)
    return fail(h, DCX_ERR_HIP, "reading VQ rescore counters failed");
  if (rows_rescored) *rows_rescored = v[0];
  if (codes_rescored) *codes_rescored = v[1];
  if (reset && hipMemset(h->vq_stats, 0, sizeof v) != hipSuccess)
    return fail(h, DCX_ERR_HIP, "resetting VQ rescore counters failed");
  return DCX_OK;
}

int32_t dcx_profile_count(const dcx_codec* h) { return h ? (int32_t)h->prof_names.size() : 0; }

int dcx_profile_read(dcx_codec* h, int32_t i, const char** name, int64_t* launches, double* ms, double* flops,
                     double* bytes) {
  if (!h) return DCX_ERR_INVALID_ARG;
  prof_collect(h);
  if (i < 0 || i >= (int32_t)h->prof_names.size()) return DCX_ERR_INVALID_ARG;
  if (name) *name = h->prof_names[i].c_str();
  if (launches) *launches = h->prof_launches[i];
  if (ms) *ms = h->prof_ms[i];
  if (flops) *flops = h->prof_flops[i];
  if (bytes) *bytes = h->prof_bytes[i];
  return DCX_OK;
}

}  // extern "C"
