"""Streaming encode -> decode in fixed hops with the whole hop captured in one HIP graph (C5).

BASELINE.json configs[4] / SURVEY.md §8(d) C5: 1 s hops (24,000 samples -> 93 frames -> 23,808
output samples), B = 1, one hipGraph-captured step, p50/p99 latency. Each hop is encoded and
decoded on its own, exactly as the reference does for a 1 s clip
(`DistilCodec.encode` + `decode_from_codes`, distil_codec.py:545-594). `HaloStream` below is the
halo-overlapped variant whose chunked output equals the full-clip output.
`TokenStream` is the other direction for many sessions at once: codes -> audio while the codes are
still arriving, one dcx_stream_decode_step per push (DESIGN.md §3 "Token streams"); `AudioStream` is
its mirror, audio -> codes for many sessions, one dcx_stream_encode_step per push ("Audio streams").

The C-ABI stage calls allocate nothing and never synchronise (include/distilcodec_amd.h), so a
whole `dcx_encode_decode` call is captured by `torch.cuda.graph` as it is launched: every kernel
on the capture stream, and the workspace and outputs fixed before capture.
"""
from __future__ import annotations

import torch

from .engine import NativeCodec


class GraphedHop:
    """One captured encode->decode step for `batch` hops of `hop_samples` samples each.

    Each hop is preprocessed like a clip of that length (`preprocess_raw_audio_batch`,
    distil_codec.py:133-136): one zero sample in front, so the static input holds
    hop_samples + 1 samples. `__call__(chunk)` copies the chunk in after the pad, replays the graph
    on the current stream and returns the static (codes, wav) outputs. The next call overwrites
    them, so clone them to keep them.
    """

    def __init__(self, engine: NativeCodec, hop_samples: int = 24000, batch: int = 1):
        self.engine = engine
        self.device = engine.device
        self.hop_samples = hop_samples
        self.batch = batch
        self.frames = engine.num_frames(hop_samples + 1)
        self.audio = torch.zeros(batch, hop_samples + 1, device=self.device)  # [:, 0] stays 0
        self.codes = torch.empty(engine._codes_shape(batch, self.frames), dtype=torch.int32, device=self.device)
        self.wav = torch.empty(batch, engine.hop * self.frames, device=self.device)
        # The graph records raw pointers, so it owns its workspace: the engine's shared buffer is
        # reallocated whenever a later call on the same engine needs more (a longer clip, a
        # HaloStream window), which would leave replays writing into freed memory.
        self.ws = torch.empty(engine.workspace_size(batch, self.frames), dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            # one eager run (module loading, first-launch work) on a side stream, then capture
            s = torch.cuda.Stream(self.device)
            s.wait_stream(torch.cuda.current_stream(self.device))
            with torch.cuda.stream(s):
                engine.encode_decode(self.audio, self.codes, self.wav, ws=self.ws)
            torch.cuda.current_stream(self.device).wait_stream(s)
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                engine.encode_decode(self.audio, self.codes, self.wav, ws=self.ws)

    def __call__(self, chunk: torch.Tensor):
        if tuple(chunk.shape) != (self.batch, self.hop_samples):
            raise ValueError(f"expected a chunk of shape {(self.batch, self.hop_samples)}, got {tuple(chunk.shape)}")
        self.audio[:, 1:].copy_(chunk, non_blocking=True)
        self.graph.replay()
        return self.codes, self.wav


def receptive_field(cfg: dict) -> tuple[int, int]:
    """(encoder, decoder) half receptive fields in frames, rounded up, for the architecture in `cfg`
    (about ±60 and ±21).  Encoder: the stem conv plus one depthwise conv
    per ConvNeXt block (encoders.py:21-60) and the quantizer's down block (grfvq.py:105-132).
    Decoder: the quantizer's up block, conv_pre, each stage's ConvTranspose and ResBlocks
    (generators.py:29-147), conv_post, each converted to frames at its stage's rate."""
    import math

    enc, q, dec = cfg["encoder"], cfg["quantizer"], cfg["decoder"]
    dw = 3  # ConvNeXt depthwise k7
    e = enc.get("kernel_size", 7) // 2 + dw * sum(enc["depths"]) + dw  # + the down block
    hop = 1
    for r in dec["upsample_rates"]:
        hop *= r
    d = dw + dec.get("pre_conv_kernel_size", 13) // 2  # up block + conv_pre (frame rate)
    rate = 1
    for r, k in zip(dec["upsample_rates"], dec["upsample_kernel_sizes"]):
        d += math.ceil(k / r / 2) / rate  # ConvTranspose: its input samples, at `rate` per frame
        rate *= r
        res = max(sum(dd * (kk - 1) // 2 + (kk - 1) // 2 for dd in dils)
                  for kk, dils in zip(dec["resblock_kernel_sizes"], dec["resblock_dilation_sizes"]))
        d += res / rate
    d += dec.get("post_conv_kernel_size", 13) // 2 / hop
    return int(e), int(math.ceil(d))


class _SlotStream:
    """What TokenStream and AudioStream share: the step's inputs (a payload of 32-bit words, then the
    slots' counts and flags) as views of one device buffer, staged through a few pinned host buffers
    in turn and uploaded in one copy, so a push never waits for the device; and the step run eagerly
    or as one captured HIP graph over the stream's static tensors.  A subclass provides `_step()`
    (the native step on its tensors) and `_reset()` (its state emptied)."""

    FINAL, RESTART = 1, 2

    def _init_io(self, n_words: int):
        B, dev = self.sessions, self.engine.device
        self._n_words = n_words
        self._in = torch.zeros(n_words + 2 * B, dtype=torch.int32, device=dev)
        # (each host buffer is reused once its own upload has run)
        self._hosts = [torch.zeros(n_words + 2 * B, dtype=torch.int32).pin_memory() for _ in range(4)]
        self._uploaded = [None] * len(self._hosts)
        self._turn = 0
        self.n_new, self.flags = self._in[n_words:n_words + B], self._in[n_words + B:]
        self.graph = None

    def _capture(self):
        dev = self.engine.device
        with torch.cuda.device(dev):
            s = torch.cuda.Stream(dev)  # eager warm-up (first-launch work) off the capture
            s.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(s):
                self._step()  # every slot pushes nothing: the counters stay 0
                self._reset()
            torch.cuda.current_stream(dev).wait_stream(s)
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                self._step()

    def _flags_of(self, n_entries: int, final, restart) -> list:
        B = self.sessions
        if n_entries != B:
            raise ValueError(f"expected one entry per slot ({B}), got {n_entries}")
        final, restart = set(final), set(restart)
        if not (final | restart) <= set(range(B)):
            raise ValueError(f"final / restart name slots outside [0, {B})")
        return [(self.FINAL if b in final else 0) | (self.RESTART if b in restart else 0) for b in range(B)]

    def _upload_and_run(self, payload, counts, flags):
        """payload: the step's int32 words (a flat numpy view), staged with counts and flags, uploaded
        in one copy; then the step."""
        B, n = self.sessions, self._n_words
        k = self._turn
        self._turn = (k + 1) % len(self._hosts)
        if self._uploaded[k] is not None:
            self._uploaded[k].synchronize()  # the upload of four pushes ago
        host = self._hosts[k].numpy()
        host[:n] = payload
        host[n:n + B] = counts
        host[n + B:] = flags
        with torch.cuda.device(self.engine.device):
            self._in.copy_(self._hosts[k], non_blocking=True)
            self._uploaded[k] = torch.cuda.Event()
            self._uploaded[k].record()
        if self.graph is not None:
            self.graph.replay()
        else:
            self._step()


class TokenStream(_SlotStream):
    """Batched streaming decode, codes -> audio (DESIGN.md §3 "Token streams"): `sessions` utterances
    that each grow by at most `push_frames` frames per `push`, decoded together in one
    dcx_stream_decode_step per push, every slot's samples those of its full-clip decode up to fp32
    summation order.  A frame's audio is returned once `halo_frames` codes after it have arrived
    (default: the decoder's half receptive field, `receptive_field(cfg)[1]`), or when the slot is
    marked `final`; the slot's state lives on the device, and the slots' counters are mirrored on the
    host (dcx_stream_plan_step), so `push` reads nothing back and never synchronises.

    `graph=True` captures the step once in a HIP graph over the stream's static tensors and replays
    it per push, bit-equal to the eager step.  `n_invalid` (device int32 [1]) counts pushed codes
    outside the codebook; it stays 0 after the host-side validation `push` does.
    """

    UNUSED = 1 << 20  # fills the entries of new_codes beyond a slot's count: never read

    def __init__(self, engine: NativeCodec, sessions: int, push_frames: int, halo_frames: int | None = None,
                 graph: bool = False, token_id_offset: int = 0):
        self.engine = engine
        self.sessions, self.push_frames = int(sessions), int(push_frames)
        self.halo_frames = receptive_field(engine.cfg)[1] if halo_frames is None else int(halo_frames)
        self.token_id_offset = token_id_offset
        B, P, h, R, dev = self.sessions, self.push_frames, self.halo_frames, engine.R, engine.device
        self.state = engine.stream_state(B, P, h)  # ValueError for a bad geometry
        n_codes = B * P * R
        self._init_io(n_codes)
        self.new_codes = self._in[:n_codes].view(engine._codes_shape(B, P))
        self.wav_out = torch.zeros(B, engine.hop * (P + h), device=dev)
        self.n_out = torch.zeros(B, dtype=torch.int32, device=dev)
        self.n_invalid = torch.zeros(1, dtype=torch.int32, device=dev)
        self.ws = torch.empty(engine.workspace_size(B, P + 2 * h), dtype=torch.uint8, device=dev)
        self._slots = [(0, 0, 0)] * B  # host mirror of (T, E, closed)
        if graph:
            self._capture()

    def _step(self):
        self.engine.stream_step(self.state, self.sessions, self.push_frames, self.halo_frames, self.new_codes, self.n_new,
                                self.flags, self.wav_out, self.n_out, self.n_invalid, ws=self.ws)

    def _reset(self):
        self.engine.stream_reset(self.state, self.sessions, self.push_frames, self.halo_frames)

    def slot(self, b: int) -> tuple[int, int, bool]:
        """(codes received, frames emitted, closed) of slot b, from the host mirror."""
        T, E, closed = self._slots[b]
        return T, E, bool(closed)

    def push(self, codes_per_slot, final=(), restart=()) -> list:
        """One step.  `codes_per_slot`: per slot, None or the new frames' codes, [n] ([n, R] for R > 1
        codebooks), n <= push_frames; `final` / `restart`: the slots that end with this push / start
        a new utterance with it.  Returns one 1-D tensor of the 256 take samples that became final per
        slot.  ValueError for too many frames or a wrong shape, RuntimeError for codes pushed to a
        closed slot without `restart`, IndexError for a code outside the codebook: all before any
        upload, so a refused push changes nothing."""
        import numpy as np

        eng, B, P, R = self.engine, self.sessions, self.push_frames, self.engine.R
        flags = self._flags_of(len(codes_per_slot), final, restart)
        stage = np.full((B, P, R), self.UNUSED, dtype=np.int32)
        counts = [0] * B
        for b, c in enumerate(codes_per_slot):
            if c is None:
                continue
            c = np.asarray(c.cpu() if isinstance(c, torch.Tensor) else c)
            if c.ndim == 1 and R == 1:
                c = c[:, None]
            if c.ndim != 2 or c.shape[1] != R:
                raise ValueError(f"slot {b}: codes must be shaped {eng._codes_shape('n')}, got {tuple(c.shape)}")
            n = c.shape[0]
            if n > P:
                raise ValueError(f"slot {b}: {n} frames exceed push_frames={P}")
            if n and self._slots[b][2] and not flags[b] & self.RESTART:
                raise RuntimeError(f"slot {b} is closed: pass it in `restart` to start a new utterance")
            if n and (int(c.min()) < 0 or int(c.max()) >= eng.NC):
                raise IndexError(f"slot {b}: audio code out of range for a codebook of {eng.NC} entries")
            stage[b, :n] = c
            counts[b] = n
        self._upload_and_run(stage.reshape(-1), counts, flags)
        out = self.wav_out.clone()  # the static output is overwritten by the next push
        outs = []
        for b in range(B):
            T, E, closed, _, _, take = eng.stream_plan_step(self.halo_frames, P, *self._slots[b], counts[b], flags[b])
            self._slots[b] = (T, E, closed)
            outs.append(out[b, :eng.hop * take])
        return outs

    def push_tokens(self, token_ids_per_slot, final=(), restart=(), minus_token_offset: bool = True) -> list:
        """`push` for the flat frame-major LLM token ids `DistilCodec.encode` yields (R ids per frame;
        ValueError for a list that is not a multiple of R), `token_id_offset` subtracted as
        `decode_from_codes` does.  Returns one (1, 1, n) tensor per slot."""
        import numpy as np

        R, off = self.engine.R, self.token_id_offset if minus_token_offset else 0
        codes = []
        for b, ids in enumerate(token_ids_per_slot):
            if ids is None:
                codes.append(None)
                continue
            a = np.asarray(ids, dtype=np.int64).reshape(-1)
            if a.size % R:
                raise ValueError(f"slot {b}: a code list of {a.size} entries is not a multiple of the {R} codebooks per frame")
            codes.append((a - off).reshape(-1, R))
        return [w[None, None, :] for w in self.push(codes, final=final, restart=restart)]


class AudioStream(_SlotStream):
    """Batched streaming tokenization, audio -> codes (DESIGN.md §3 "Audio streams"), the mirror of
    TokenStream: `sessions` utterances that each grow by at most `push_samples` raw samples per `push`,
    tokenized together in one dcx_stream_encode_step per push, every slot's codes those of its full
    clip (`tokenize_ragged` of the clip alone) up to fp32 summation order.  A frame's code is returned
    once `halo_frames` mel frames after it exist that touch no reflected sample (default: the encoder's
    half receptive field, `receptive_field(cfg)[0]`), or when the slot is marked `final`, where the
    window ends at the utterance's true last sample.  The slots' state lives on the device and their
    counters are mirrored on the host (dcx_stream_encode_plan_step), so `push` reads nothing back.

    `graph=True` captures the step once in a HIP graph and replays it per push, bit-equal to the eager
    step.  `want_pjt_in`: every push also leaves the emitted frames' x_pjt_in rows in `pjt_in_out`.
    """

    MIN_SAMPLES = 384  # an utterance needs the reflect pad's length

    def __init__(self, engine: NativeCodec, sessions: int, push_samples: int, halo_frames: int | None = None,
                 graph: bool = False, want_pjt_in: bool = False, token_id_offset: int = 0, token_table: dict | None = None):
        self.engine = engine
        self.token_table = token_table  # tokens.construct_audio_code's table (push_tokens)
        self.sessions, self.push_samples = int(sessions), int(push_samples)
        self.halo_frames = receptive_field(engine.cfg)[0] if halo_frames is None else int(halo_frames)
        self.want_pjt_in = bool(want_pjt_in)
        self.token_id_offset = token_id_offset
        B, P, h, dev = self.sessions, self.push_samples, self.halo_frames, engine.device
        self.state = engine.audio_stream_state(B, P, h, self.want_pjt_in)  # ValueError for a bad geometry
        self.window_samples, self.window_frames, self.out_frames = engine.audio_stream_geometry(P, h)
        self._init_io(B * P)
        self.new_samples = self._in[:B * P].view(torch.float32).view(B, P)
        self.codes_out = torch.full(engine._codes_shape(B, self.out_frames), -1, dtype=torch.int32, device=dev)
        self.n_out = torch.zeros(B, dtype=torch.int32, device=dev)
        self.pjt_in_out = torch.zeros(B, self.out_frames, engine.CD, device=dev) if self.want_pjt_in else None
        self.ws = torch.empty(engine.audio_stream_workspace_size(B, P, h), dtype=torch.uint8, device=dev)
        self._slots = [(0, 0, 0)] * B  # host mirror of (M, C, closed)
        if graph:
            self._capture()

    def _step(self):
        self.engine.audio_stream_step(self.state, self.sessions, self.push_samples, self.halo_frames, self.new_samples,
                                      self.n_new, self.flags, self.codes_out, self.n_out, self.pjt_in_out, ws=self.ws)

    def _reset(self):
        self.engine.audio_stream_reset(self.state, self.sessions, self.push_samples, self.halo_frames, self.want_pjt_in)

    def slot(self, b: int) -> tuple[int, int, bool]:
        """(samples received, codes emitted, closed) of slot b, from the host mirror."""
        M, C, closed = self._slots[b]
        return M, C, bool(closed)

    def push(self, chunks_per_slot, final=(), restart=()) -> list:
        """One step.  `chunks_per_slot`: per slot, None or the new raw samples (1-D, at most
        push_samples); `final` / `restart`: the slots that end with this push / start a new utterance
        with it.  Returns one int32 tensor [take] ([take, R] for R > 1 codebooks) per slot: the codes
        that became final.  ValueError for a chunk above push_samples or a `final` that would leave
        an utterance of fewer than 384 samples, RuntimeError for samples pushed to a closed slot
        without `restart`: all before any upload, so a refused push changes nothing."""
        import numpy as np

        eng, B, P = self.engine, self.sessions, self.push_samples
        flags = self._flags_of(len(chunks_per_slot), final, restart)
        stage = np.full((B, P), np.nan, dtype=np.float32)  # entries beyond a slot's count: never read
        counts = [0] * B
        for b, c in enumerate(chunks_per_slot):
            if c is not None:
                c = np.asarray(c.cpu() if isinstance(c, torch.Tensor) else c, dtype=np.float32).reshape(-1)
                n = c.shape[0]
                if n > P:
                    raise ValueError(f"slot {b}: a chunk of {n} samples exceeds push_samples={P}")
                if n and self._slots[b][2] and not flags[b] & self.RESTART:
                    raise RuntimeError(f"slot {b} is closed: pass it in `restart` to start a new utterance")
                stage[b, :n] = c
                counts[b] = n
            M, _, closed = (0, 0, 0) if flags[b] & self.RESTART else self._slots[b]
            if flags[b] & self.FINAL and not closed and M + counts[b] < self.MIN_SAMPLES:
                raise ValueError(f"slot {b}: final on an utterance of {M + counts[b]} samples, fewer than the "
                                 f"{self.MIN_SAMPLES} the reflect pad needs")
        self._upload_and_run(stage.reshape(-1).view(np.int32), counts, flags)
        out = self.codes_out.clone()  # the static output is overwritten by the next push
        outs = []
        for b in range(B):
            M, C, closed, _, _, _, take = eng.audio_stream_plan_step(self.halo_frames, P, *self._slots[b], counts[b], flags[b])
            self._slots[b] = (M, C, closed)
            outs.append(out[b, :take])
        return outs

    def push_tokens(self, chunks_per_slot, final=(), restart=(), add_token_offset: bool = True) -> list:
        """`push`, returning per slot the flat frame-major LLM token ids `DistilCodec.encode` yields
        for the emitted frames (R ids per frame): the `absolute_token_id` of tokens.audio_tokenize with
        the stream's token table, or the codes plus `token_id_offset` without one; the ids
        `TokenStream.push_tokens` takes.  `add_token_offset=False`: the codes themselves."""
        from . import tokens

        outs = []
        for c in self.push(chunks_per_slot, final=final, restart=restart):
            flat = c.reshape(-1).tolist()
            if not add_token_offset:
                outs.append(flat)
            elif self.token_table is not None:
                outs.append([t["absolute_token_id"] for t in tokens.audio_tokenize(self.token_table, flat, 1, self.engine.R)])
            else:
                outs.append([x + self.token_id_offset for x in flat])
        return outs


class HaloStream:
    """Streaming encode -> decode whose output equals the full-clip result.

    `push(chunk)` appends samples and returns the waveform samples that became final; `flush()`
    ends the stream and returns the rest.  A frame's code is final once its encoder receptive field
    (`enc_halo` frames each side, plus the 2 / 3 mel frames a segment edge reflects) has arrived;
    a frame's audio is final once the codes `gen_halo` frames around it are.  Each step runs the
    stage kernels on a window: mel + encoder + VQ from `enc_halo + 2` frames before the first new
    code to the end of the received audio, and VQ decode + generator over the new frames plus
    `gen_halo` on each side.  Inside a window the clip edges are the true clip edges (the
    reference's leading zero sample, reflect padding at the end on `flush`), so every emitted
    frame sees the same inputs as in a full-clip run.  Latency: about enc_halo + gen_halo + 3
    frames of look-ahead.  Results equal the full clip up to fp32 summation order (window lengths
    pick other conv tilings).

    Fixed windows (`push_samples`): every push of at most `push_samples` samples runs on windows of
    one shape, the encoder window zero-padded past the received audio and the generator window
    padded with code 0 past the last code.  The padding only reaches frames that are not final
    yet (it sits beyond the receptive field of every emitted frame), so the output is the same
    function of the input.  `graph=True` captures the two window steps (mel -> encoder -> VQ
    search; VQ decode -> generator) in two HIP graphs and replays them, bit-equal to the eager
    fixed-window run; `flush` runs the variable-shape eager step (the clip end is reflected).
    """

    def __init__(self, engine: NativeCodec, enc_halo: int | None = None, gen_halo: int | None = None,
                 record_codes: bool = False, push_samples: int | None = None, graph: bool = False):
        self.engine = engine
        self.code_log = [] if record_codes else None  # every final code, in order (tests / token output)
        e, d = receptive_field(engine.cfg)
        self.enc_halo = e if enc_halo is None else enc_halo
        self.gen_halo = d if gen_halo is None else gen_halo
        self.hop = engine.hop
        # only the still-needed tails are kept: audio from sample a_off (a multiple of 256, in the
        # coordinates of the padded clip, whose sample 0 is the reference's leading zero), codes
        # from frame c_off
        self.audio = torch.zeros(1, device=engine.device)
        self.a_off = 0
        self.codes = torch.empty(engine._codes_shape(0), dtype=torch.int32, device=engine.device)  # [frames(, R)]
        self.c_off = 0
        self.emitted = 0  # frames whose audio was returned
        self.done = False
        self.push_samples = push_samples
        self.graphs = None
        if graph and not push_samples:
            raise ValueError("graph=True needs fixed windows: pass push_samples")
        if push_samples:
            self._init_windows(push_samples, graph)

    # ------------------------------------------------------------------ fixed windows
    def _init_windows(self, push: int, graph: bool):
        eng, hop = self.engine, self.hop
        # encoder window: received audio from frame a = (codes done) - enc_halo - 2; with codes done
        # = (mel frames of the previous audio) - enc_halo, it spans at most push + 639 + hop (2 e + 2)
        # samples (the first pushes, a = 0, span less)
        self.n_enc = push + 640 + hop * (2 * self.enc_halo + 2)
        # generator window: the frames that became final (at most ceil(push / hop) + 1) and gen_halo
        # on each side
        self.t_gen = -(-push // hop) + 1 + 2 * self.gen_halo
        dev = eng.device
        self.a_win = torch.zeros(1, self.n_enc, device=dev)
        self.c_win = torch.zeros(eng._codes_shape(1, self.t_gen), dtype=torch.int32, device=dev)
        t_enc = eng.num_frames(self.n_enc)
        self.ws = torch.empty(max(eng.workspace_size(1, t_enc), eng.workspace_size(1, self.t_gen)),
                              dtype=torch.uint8, device=dev)
        self.codes_win = self.wav_win = None
        if graph:
            with torch.cuda.device(dev):
                s = torch.cuda.Stream(dev)  # eager warm-up (first-launch work) off the capture
                s.wait_stream(torch.cuda.current_stream(dev))
                with torch.cuda.stream(s):
                    self._enc_body()
                    self._gen_body()
                torch.cuda.current_stream(dev).wait_stream(s)
                g_enc, g_gen = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
                with torch.cuda.graph(g_enc):
                    self.codes_win = self._enc_body()
                with torch.cuda.graph(g_gen):
                    self.wav_win = self._gen_body()
            self.graphs = (g_enc, g_gen)

    def _enc_body(self):
        eng = self.engine
        feat = eng.encode(eng.mel(self.a_win, ws=self.ws), ws=self.ws)
        return eng.vq_encode(feat, want_pjt_in=False, want_fup=False, want_quantized=False, ws=self.ws)[0]

    def _gen_body(self):
        eng = self.engine
        return eng.generate(eng.vq_decode(self.c_win, ws=self.ws), ws=self.ws)

    def _encode_window(self, seg: torch.Tensor, final: bool) -> torch.Tensor:
        """Codes of the window whose audio is seg (from its first sample on)."""
        eng = self.engine
        if self.push_samples is None or final:
            return eng.vq_encode(eng.encode(eng.mel(seg.unsqueeze(0))), want_pjt_in=False, want_fup=False,
                                 want_quantized=False)[0][0]
        n = seg.numel()
        if n > self.n_enc:
            raise ValueError(f"push larger than the fixed window allows (push_samples={self.push_samples})")
        self.a_win[0, :n].copy_(seg)
        self.a_win[0, n:].zero_()
        if self.graphs:
            self.graphs[0].replay()
            return self.codes_win[0]
        return self._enc_body()[0]

    def _generate_window(self, codes: torch.Tensor, final: bool) -> torch.Tensor:
        eng = self.engine
        if self.push_samples is None or final:
            return eng.generate(eng.vq_decode(codes.unsqueeze(0)))[0]
        n = codes.shape[0]
        if n > self.t_gen:
            raise ValueError(f"push larger than the fixed window allows (push_samples={self.push_samples})")
        self.c_win[0, :n].copy_(codes)
        self.c_win[0, n:].zero_()
        if self.graphs:
            self.graphs[1].replay()
            return self.wav_win[0]
        return self._gen_body()[0]

    # ------------------------------------------------------------------ stream
    @property
    def n_codes(self) -> int:
        return self.c_off + self.codes.shape[0]

    def _final_codes(self, final: bool) -> int:
        n = self.a_off + self.audio.numel()
        if final:
            return self.engine.num_frames(n)
        avail = (n - 640) // 256 + 1 if n >= 640 else 0  # mel frames with no reflected sample
        return max(0, avail - self.enc_halo)

    def _advance(self, final: bool) -> torch.Tensor:
        eng = self.engine
        c_done, c_new = self.n_codes, self._final_codes(final)
        if c_new > c_done:
            a = max(0, c_done - self.enc_halo - 2)
            seg = self.audio[256 * a - self.a_off:]
            codes = self._encode_window(seg, final)
            new_codes = codes[c_done - a:c_new - a].clone()
            self.codes = torch.cat([self.codes, new_codes])
            if self.code_log is not None:
                self.code_log.append(new_codes)
            keep = 256 * max(0, c_new - self.enc_halo - 2)  # the next window's first sample
            self.audio = self.audio[keep - self.a_off:]
            self.a_off = keep
        T = self.n_codes
        f_new = T if final else max(self.emitted, T - self.gen_halo)
        if f_new <= self.emitted:
            return torch.empty(0, device=eng.device)
        g0, g1 = max(0, self.emitted - self.gen_halo), min(T, f_new + self.gen_halo)
        wav = self._generate_window(self.codes[g0 - self.c_off:g1 - self.c_off], final)
        out = wav[self.hop * (self.emitted - g0):self.hop * (f_new - g0)].clone()
        self.emitted = f_new
        drop = max(0, f_new - self.gen_halo) - self.c_off
        self.codes, self.c_off = self.codes[drop:], self.c_off + drop
        return out

    def push(self, chunk) -> torch.Tensor:
        if self.done:
            raise RuntimeError("push after flush")
        chunk = torch.as_tensor(chunk, dtype=torch.float32).to(self.engine.device).reshape(-1)
        if self.push_samples is not None and chunk.numel() > self.push_samples:
            raise ValueError(f"chunk of {chunk.numel()} samples exceeds push_samples={self.push_samples}")
        self.audio = torch.cat([self.audio, chunk])
        return self._advance(final=False)

    def flush(self) -> torch.Tensor:
        self.done = True
        return self._advance(final=True)
