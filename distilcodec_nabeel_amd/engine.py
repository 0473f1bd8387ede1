"""Device-side engine: one libdcx handle per GPU, torch tensors as device buffers.

Every method is stream-ordered on `torch.cuda.current_stream(device)` and hands raw device
pointers to the C ABI.  Tensors are channels-last ([B][T][C]) as the kernels produce them.
"""
from __future__ import annotations

import contextlib
import ctypes
import os

import numpy as np
import torch

from . import _native
from .config import check_supported


# codebook EMA statistics a trained checkpoint carries (vector_quantize_pytorch.py:508-531); eval
# never reads them, and embed_avg alone is as large as the codebook (470 MB), so they are not copied
_TRAINING_ONLY = ("_codebook.embed_avg", "_codebook.cluster_size")

# dcx_set_knob switches and their shipped values (include/distilcodec_amd.h; dcx::Knobs)
KNOB_DEFAULTS = {
    "DCX_RP_R": 0, "DCX_RP_OLD": 0, "DCX_RP_G64": 0, "DCX_GELU_LUT": -1,
    "DCX_BF16_PERSIST": 1, "DCX_BF16_REG_EPI": 1, "DCX_DWCONV_TILED": 0, "DCX_SPLIT_MIN_STEPS": 0,
    "DCX_SPLIT_GROUP_OFF": 0, "DCX_H3": 1, "DCX_H3_BN": 0, "DCX_H3_1X1": 1, "DCX_H3_SPLIT": 1, "DCX_H3_PAIRS": 1, "DCX_RP_RING": 1,
    "DCX_ENC_STREAMS": 2, "DCX_EPI_GENERIC": 0, "DCX_CONV_GROUP": 1,
}

GEMM_MODES = {"f32": _native.DCX_GEMM_F32, "x6": _native.DCX_GEMM_X6, "bf16": _native.DCX_GEMM_BF16}


class NativeCodec:
    """`gemm`: "x6" (default; fp32 operands as three bf16 planes, six exact products, fp32
    accumulation), "f32" (v_mfma_f32_32x32x2_f32) or "bf16" (the reference's enable_bfloat16:
    bf16 operands and results, fp32 accumulation; see DCX_GEMM_BF16).  Env DCX_GEMM overrides
    the default."""

    def __init__(self, cfg: dict, state: dict, device, with_generator: bool = True, gemm: str | None = None):
        check_supported(cfg)
        self.cfg = cfg
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _native.NativeUnavailable("the DistilCodec MI355X path needs a GPU device (cuda:N on ROCm)")
        if not torch.cuda.is_available():
            raise _native.NativeUnavailable("no GPU visible to torch: the HIP path cannot run here")
        self.L = _native.lib()
        self.c = _native.config_from_dict(cfg)
        self.D = cfg["quantizer"]["input_dim"]
        self.CD = cfg["quantizer"]["codebook_dim"]
        self.NC = cfg["quantizer"]["codebook_size"]
        self.n_mels = cfg["spec_transform"]["num_mels"]
        self.hop = cfg["spec_transform"]["hop_size"]
        self.with_generator = with_generator
        self._ws = None
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            self._check(self.L.dcx_create(ctypes.byref(self.c), ctypes.byref(h)), None)
            self.h = h
            self.gemm = gemm or os.environ.get("DCX_GEMM", "x6")
            if self.gemm not in GEMM_MODES:
                raise ValueError(f"unknown GEMM mode {self.gemm!r}; expected one of {sorted(GEMM_MODES)}")
            self._check(self.L.dcx_set_gemm_mode(self.h, GEMM_MODES[self.gemm]))
            # residual codebooks (ResidualVQ): codes carry an innermost axis of R entries when R > 1
            self._check(self.L.dcx_set_num_codebooks(self.h, int(cfg["quantizer"]["n_codebooks"])))
            self.R = int(self.L.dcx_num_codebooks(self.h))
            for part in ("encoder", "quantizer") + (("generator",) if with_generator else ()):
                for k, v in state[part].items():
                    if k.endswith(_TRAINING_ONLY):
                        continue
                    a = np.ascontiguousarray(np.asarray(v, dtype=np.float32))
                    shape = (ctypes.c_int64 * max(a.ndim, 1))(*a.shape)
                    self._check(self.L.dcx_set_tensor(self.h, f"{part}.{k}".encode(), a.ctypes.data_as(ctypes.c_void_p),
                                                      a.ndim, shape))
            self._check(self.L.dcx_finalize(self.h, 1 if with_generator else 0))

    # ------------------------------------------------------------------ plumbing
    def _check(self, rc, h="self"):
        if rc == _native.DCX_OK:
            return
        msg = ""
        handle = self.h if h == "self" else h
        if handle:
            msg = self.L.dcx_last_error(handle).decode()
        msg = msg or self.L.dcx_status_string(rc).decode()
        if rc == _native.DCX_ERR_INVALID_ARG:
            raise ValueError(msg)
        if rc == _native.DCX_ERR_MISSING_WEIGHT:
            raise KeyError(msg)
        raise _native.NativeError(rc, msg)

    def __del__(self):
        h = getattr(self, "h", None)
        if h:
            try:
                self.L.dcx_destroy(h)
            except Exception:
                pass
            self.h = None

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def workspace_size(self, batch: int, frames: int) -> int:
        return int(self.L.dcx_workspace_size(self.h, batch, frames))

    def workspace(self, batch: int, frames: int, ws: torch.Tensor | None = None) -> torch.Tensor:
        """The workspace of one stage call.  A caller-owned `ws` (e.g. the one a captured hipGraph
        was recorded with) is checked and used as is; otherwise the engine's shared buffer, which
        grows (is reallocated) when a call needs more."""
        return self._workspace_of(self.workspace_size(batch, frames), ws)

    def _workspace_of(self, need: int, ws: torch.Tensor | None) -> torch.Tensor:
        if ws is not None:
            if ws.device != self.device or ws.dtype != torch.uint8 or not ws.is_contiguous() or ws.numel() < need:
                raise ValueError(f"workspace must be a contiguous uint8 tensor on {self.device} of >= {need} bytes")
            return ws
        if self._ws is None or self._ws.numel() < need:
            self._ws = None
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._ws

    def _codes_shape(self, *lead) -> tuple:
        """Shape of a codes tensor: `lead` alone for one codebook, `lead + (R,)` for a chain."""
        return tuple(lead) if self.R == 1 else tuple(lead) + (self.R,)

    def _codes_in(self, codes) -> torch.Tensor:
        """A caller's codes as int32 on the device, [B, T] (R == 1) or [B, T, R]."""
        codes = self._dev(codes, torch.int32)
        want = 2 if self.R == 1 else 3
        if codes.ndim != want or (self.R > 1 and codes.shape[2] != self.R):
            raise ValueError(f"codes must be shaped {self._codes_shape('B', 'T')}, got {tuple(codes.shape)}")
        return codes

    @staticmethod
    def _ptr(t):
        return ctypes.c_void_p(t.data_ptr()) if t is not None else None

    def _dev(self, t, dtype):
        t = torch.as_tensor(t)
        if t.device != self.device or t.dtype != dtype or not t.is_contiguous():
            t = t.to(device=self.device, dtype=dtype).contiguous()
        return t

    def set_gemm(self, mode: str) -> None:
        self._check(self.L.dcx_set_gemm_mode(self.h, GEMM_MODES[mode]))
        self.gemm = mode

    def set_split_k(self, max_splits: int) -> None:
        """Split-K latency mode (dcx_set_split_k): few-tile convs run as up to `max_splits` K-slices.
        Opt-in for small batches; results then depend on the tile count (not batch-invariant)."""
        self._check(self.L.dcx_set_split_k(self.h, int(max_splits)))
        self._ws = None  # the workspace size changed

    def set_knob(self, name: str, value: int) -> None:
        """A/B and test switch of the kernel selection (dcx_set_knob; names are the DCX_* environment
        variables dcx_create reads once).  Takes effect for later calls on this engine."""
        self._check(self.L.dcx_set_knob(self.h, name.encode(), int(value)))

    def get_knob(self, name: str) -> int:
        """The current value of a switch (dcx_get_knob)."""
        v = ctypes.c_int32(0)
        self._check(self.L.dcx_get_knob(self.h, name.encode(), ctypes.byref(v)))
        return v.value

    @contextlib.contextmanager
    def knobs(self, **values):
        """Switches set for the calls inside the block, then back to the values they had before
        (an environment override given at creation included): `with eng.knobs(DCX_RP_OLD=1): ...`."""
        saved = {k: self.get_knob(k) for k in values}
        for k, v in values.items():
            self.set_knob(k, v)
        try:
            yield self
        finally:
            for k, v in saved.items():
                self.set_knob(k, v)

    def epi_form_launches(self, reset: bool = False) -> list[int]:
        """Launches of the wide h3 conv kernels in this process by epilogue form (dcx_epi_form_launches):
        nine compile-time forms, then the run-time epilogue."""
        v = (ctypes.c_int64 * 10)()
        self._check(self.L.dcx_epi_form_launches(v, 10, int(reset)))
        return list(v)

    def range_flags(self, reset: bool = False) -> int:
        """The h3 range flags (dcx_range_flags; synchronises): bit 0 a non-finite operand bound, bit 1
        a saturated h3 operand.  0 for every finite input."""
        v = ctypes.c_int32(0)
        self._check(self.L.dcx_range_flags(self.h, ctypes.byref(v), int(reset)))
        return v.value

    def num_frames(self, n_samples: int) -> int:
        return int(self.L.dcx_num_frames(self.h, n_samples))

    # ------------------------------------------------------------------ stages
    # Every stage takes an optional caller-owned workspace `ws` (see `workspace`): a captured hipGraph
    # must keep the buffer it was recorded with.
    def mel(self, audio: torch.Tensor, ws: torch.Tensor | None = None, linear: bool = False):
        """audio (B, N) fp32 (with the reference's leading zero) -> mel (B, T, n_mels); with
        `linear`, also log(clamp(|STFT|, 1e-5)) (B, T, n_fft/2 + 1) (return_linear, mel_spec.py:119-120)."""
        audio = self._dev(audio, torch.float32)
        B, N = audio.shape
        T = self.num_frames(N)
        out = torch.empty(B, T, self.n_mels, device=self.device)
        ws = self.workspace(B, T, ws)
        with torch.cuda.device(self.device):
            if linear:
                lin = torch.empty(B, T, self.cfg["spec_transform"]["n_fft"] // 2 + 1, device=self.device)
                self._check(self.L.dcx_mel_linear(self.h, self._ptr(audio), B, N, self._ptr(out), self._ptr(lin),
                                                  self._ptr(ws), ws.numel(), self._stream()))
                return out, lin
            self._check(self.L.dcx_mel(self.h, self._ptr(audio), B, N, self._ptr(out), self._ptr(ws), ws.numel(), self._stream()))
        return out

    def encode(self, mel: torch.Tensor, ws: torch.Tensor | None = None) -> torch.Tensor:
        mel = self._dev(mel, torch.float32)
        B, T, _ = mel.shape
        out = torch.empty(B, T, self.cfg["encoder"]["dims"][-1], device=self.device)
        ws = self.workspace(B, T, ws)
        with torch.cuda.device(self.device):
            self._check(self.L.dcx_encode(self.h, self._ptr(mel), B, T, self._ptr(out), self._ptr(ws), ws.numel(), self._stream()))
        return out

    def vq_encode(self, feat: torch.Tensor, want_pjt_in=True, want_fup=True, want_quantized=True,
                  ws: torch.Tensor | None = None):
        feat = self._dev(feat, torch.float32)
        B, T, _ = feat.shape
        codes = torch.empty(self._codes_shape(B, T), dtype=torch.int32, device=self.device)
        pin = torch.empty(B, T, self.CD, device=self.device) if want_pjt_in else None
        fup = torch.empty(B, T, self.CD, device=self.device) if want_fup else None
        q = torch.empty(B, T, self.D, device=self.device) if want_quantized else None
        ws = self.workspace(B, T, ws)
        with torch.cuda.device(self.device):
            self._check(self.L.dcx_vq_encode(self.h, self._ptr(feat), B, T, self._ptr(codes), self._ptr(pin), self._ptr(fup),
                                             self._ptr(q), self._ptr(ws), ws.numel(), self._stream()))
        return codes, pin, fup, q

    def vq_decode(self, codes: torch.Tensor, ws: torch.Tensor | None = None) -> torch.Tensor:
        codes = self._codes_in(codes)
        B, T = codes.shape[:2]
        z = torch.empty(B, T, self.D, device=self.device)
        ws = self.workspace(B, T, ws)
        with torch.cuda.device(self.device):
            self._check(self.L.dcx_vq_decode(self.h, self._ptr(codes), B, T, self._ptr(z), None, self._ptr(ws), ws.numel(),
                                             self._stream()))
        return z

    def generate(self, z: torch.Tensor, ws: torch.Tensor | None = None) -> torch.Tensor:
        if not self.with_generator:
            raise RuntimeError("this engine was built without generator weights")
        z = self._dev(z, torch.float32)
        B, T, _ = z.shape
        wav = torch.empty(B, self.hop * T, device=self.device)
        ws = self.workspace(B, T, ws)
        with torch.cuda.device(self.device):
            self._check(self.L.dcx_generate(self.h, self._ptr(z), B, T, self._ptr(wav), self._ptr(ws), ws.numel(), self._stream()))
        return wav

    def encode_decode(self, audio: torch.Tensor, codes: torch.Tensor | None = None, wav: torch.Tensor | None = None,
                      ws: torch.Tensor | None = None):
        audio = self._dev(audio, torch.float32)
        B, N = audio.shape
        T = self.num_frames(N)
        if codes is None:
            codes = torch.empty(self._codes_shape(B, T), dtype=torch.int32, device=self.device)
        elif self.R > 1 and (tuple(codes.shape) != self._codes_shape(B, T) or codes.dtype != torch.int32 or not codes.is_contiguous()):
            raise ValueError(f"codes must be a contiguous int32 tensor shaped {self._codes_shape(B, T)}")
        if wav is None:
            wav = torch.empty(B, self.hop * T, device=self.device)
        ws = self.workspace(B, T, ws)
        with torch.cuda.device(self.device):
            self._check(self.L.dcx_encode_decode(self.h, self._ptr(audio), B, N, self._ptr(codes), self._ptr(wav), self._ptr(ws),
                                                 ws.numel(), self._stream()))
        return codes, wav

    def ragged_plan(self, lengths) -> tuple[np.ndarray, int, int]:
        """The plan table of a ragged batch (dcx_ragged_plan; host only): (int32 table, total samples,
        total frames) for clips of `lengths` raw samples.  ValueError names the clip that is too short."""
        n = np.ascontiguousarray(np.asarray(lengths, dtype=np.int64).reshape(-1))
        B = int(n.shape[0])
        words = int(self.L.dcx_ragged_plan_size(B))
        plan = np.zeros(max(words, 1), dtype=np.int32)
        ts, tf = ctypes.c_int64(0), ctypes.c_int64(0)
        self._check(self.L.dcx_ragged_plan(self.h, n.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), B,
                                           plan.ctypes.data_as(ctypes.c_void_p), words, ctypes.byref(ts), ctypes.byref(tf)))
        return plan, ts.value, tf.value

    def tokenize_ragged(self, clips, want_pjt_in: bool = False, want_fup: bool = False, ws: torch.Tensor | None = None):
        """Clips of different lengths (1-D tensors or arrays of raw samples, without the reference's
        leading zero) -> (codes int32 [sum T] ([sum T, R] for R > 1 codebooks), frame_offsets int64 [B + 1] (host), x_pjt_in | None,
        quantized_fup | None), the last two packed [sum T, codebook_dim].  The clips are packed back to
        back and tokenized in one call with no padding (dcx_tokenize_ragged); clip b's rows are
        [frame_offsets[b], frame_offsets[b + 1]) and equal what the clip gives alone."""
        if len(clips) == 0:
            raise ValueError("tokenize_ragged needs at least one clip")
        flat = [torch.as_tensor(c).reshape(-1) for c in clips]
        lengths = [int(c.numel()) for c in flat]
        plan, total_samples, total_frames = self.ragged_plan(lengths)
        B = len(flat)
        audio = torch.cat([c.to(device=self.device, dtype=torch.float32) for c in flat])
        plan_dev = torch.from_numpy(plan).to(self.device)
        offsets = torch.tensor(np.concatenate([[0], np.cumsum([self.num_frames(n + 1) for n in lengths])]), dtype=torch.int64)
        assert int(offsets[-1]) == total_frames
        codes = torch.empty(self._codes_shape(total_frames), dtype=torch.int32, device=self.device)
        pin = torch.empty(total_frames, self.CD, device=self.device) if want_pjt_in else None
        fup = torch.empty(total_frames, self.CD, device=self.device) if want_fup else None
        ws = self._workspace_of(int(self.L.dcx_ragged_workspace_size(self.h, B, total_frames)), ws)
        with torch.cuda.device(self.device):
            self._check(self.L.dcx_tokenize_ragged(self.h, self._ptr(audio), self._ptr(plan_dev),
                                                   plan.ctypes.data_as(ctypes.c_void_p), B, total_samples, total_frames,
                                                   self._ptr(codes), self._ptr(pin), self._ptr(fup), self._ptr(ws),
                                                   ws.numel(), self._stream()))
        return codes, offsets, pin, fup

    def slots_workspace_size(self, batch: int, slot_samples: int) -> int:
        """Workspace bytes of tokenize_slots for `batch` slots of `slot_samples` samples."""
        return int(self.L.dcx_ragged_workspace_size(self.h, batch, batch * self.num_frames(slot_samples + 1)))

    def tokenize_slots(self, audio: torch.Tensor, n_samples, want_pjt_in: bool = False, ws: torch.Tensor | None = None,
                       codes: torch.Tensor | None = None, pjt_in: torch.Tensor | None = None):
        """audio (B, Ws) raw samples (without the reference's leading zero) with per-slot sample counts
        `n_samples` -> (codes int32 (B, Wf) ((B, Wf, R) for R > 1 codebooks), x_pjt_in (B, Wf,
        codebook_dim) | None), Wf = num_frames(Ws + 1) (dcx_tokenize_slots).  Slot b's first
        num_frames(n_b + 1) rows are what the clip gives alone; codes beyond them are -1, x_pjt_in rows
        zero; a slot of fewer than 384 samples is dead.  Host lengths are validated (ValueError outside
        [0, Ws]) and uploaded; a device int32 tensor is used as it stands (a captured graph's lengths
        buffer; the kernels clamp).  `codes` / `pjt_in`: caller-owned outputs (a captured graph's)."""
        audio = self._dev(audio, torch.float32)
        if audio.ndim != 2:
            raise ValueError(f"audio must be shaped (B, Ws), got {tuple(audio.shape)}")
        B, Ws = audio.shape
        if isinstance(n_samples, torch.Tensor) and n_samples.is_cuda:
            if n_samples.dtype != torch.int32 or n_samples.numel() != B or not n_samples.is_contiguous():
                raise ValueError(f"device n_samples must be contiguous int32 [{B}]")
            n_dev = n_samples
        else:
            n = np.asarray(n_samples.cpu() if isinstance(n_samples, torch.Tensor) else n_samples, dtype=np.int64).reshape(-1)
            if n.shape[0] != B or (n < 0).any() or (n > Ws).any():
                raise ValueError(f"n_samples must hold {B} counts in [0, {Ws}]")
            n_dev = torch.from_numpy(n.astype(np.int32)).to(self.device)
        Wf = self.num_frames(Ws + 1)
        if codes is None:
            codes = torch.empty(self._codes_shape(B, Wf), dtype=torch.int32, device=self.device)
        elif tuple(codes.shape) != self._codes_shape(B, Wf) or codes.dtype != torch.int32 or not codes.is_contiguous():
            raise ValueError(f"codes must be a contiguous int32 tensor shaped {self._codes_shape(B, Wf)}")
        if pjt_in is None:
            pjt_in = torch.empty(B, Wf, self.CD, device=self.device) if want_pjt_in else None
        elif tuple(pjt_in.shape) != (B, Wf, self.CD) or pjt_in.dtype != torch.float32 or not pjt_in.is_contiguous():
            raise ValueError(f"pjt_in must be a contiguous float32 tensor shaped {(B, Wf, self.CD)}")
        ws = self._workspace_of(self.slots_workspace_size(B, Ws), ws)
        with torch.cuda.device(self.device):
            self._check(self.L.dcx_tokenize_slots(self.h, self._ptr(audio), self._ptr(n_dev), B, Ws, self._ptr(codes),
                                                  self._ptr(pjt_in), self._ptr(ws), ws.numel(), self._stream()))
        return codes, pjt_in

    def _ragged_lengths(self, lengths, B: int, T: int) -> torch.Tensor:
        """Per-clip frame counts for the ragged decode calls as a device int32 tensor.  A device
        tensor is taken as it stands (a captured graph's lengths buffer; the kernels clamp to
        [0, T]); anything else is validated on the host (ragged.check_lengths) and uploaded."""
        if isinstance(lengths, torch.Tensor) and lengths.is_cuda:
            if lengths.dtype != torch.int32 or lengths.numel() != B or not lengths.is_contiguous():
                raise ValueError(f"device lengths must be contiguous int32 [{B}]")
            return lengths
        from .ragged import check_lengths
        return torch.from_numpy(check_lengths(lengths, B, T)).to(self.device)

    def generate_ragged(self, z: torch.Tensor, lengths, ws: torch.Tensor | None = None,
                        wav: torch.Tensor | None = None) -> torch.Tensor:
        """z (B, T_max, vq_dim) fp32 with per-clip frame counts `lengths` -> wav (B, 256 T_max): clip
        b's first 256 lengths[b] samples are what the clip gives alone, the rest zeros; rows of z at
        or beyond a length are never read (dcx_generate_ragged)."""
        if not self.with_generator:
            raise RuntimeError("this engine was built without generator weights")
        z = self._dev(z, torch.float32)
        B, T, _ = z.shape
        lens = self._ragged_lengths(lengths, B, T)
        if wav is None:
            wav = torch.empty(B, self.hop * T, device=self.device)
        ws = self.workspace(B, T, ws)
        with torch.cuda.device(self.device):
            self._check(self.L.dcx_generate_ragged(self.h, self._ptr(z), self._ptr(lens), B, T, self._ptr(wav), self._ptr(ws),
                                                   ws.numel(), self._stream()))
        return wav

    def decode_ragged(self, codes: torch.Tensor, lengths, ws: torch.Tensor | None = None,
                      wav: torch.Tensor | None = None, n_invalid: torch.Tensor | None = None) -> torch.Tensor:
        """codes (B, T_max) int32 ((B, T_max, R) for R > 1 codebooks) with per-clip frame counts `lengths` -> wav (B, 256 T_max), as
        generate_ragged (dcx_decode_ragged).  Entries at or beyond a length are never read;
        n_invalid (device int32 [1], optional, zeroed by the caller) counts codes outside the
        codebook below the lengths."""
        if not self.with_generator:
            raise RuntimeError("this engine was built without generator weights")
        codes = self._codes_in(codes)
        B, T = codes.shape[:2]
        lens = self._ragged_lengths(lengths, B, T)
        if wav is None:
            wav = torch.empty(B, self.hop * T, device=self.device)
        ws = self.workspace(B, T, ws)
        with torch.cuda.device(self.device):
            self._check(self.L.dcx_decode_ragged(self.h, self._ptr(codes), self._ptr(lens), B, T, self._ptr(wav),
                                                 self._ptr(n_invalid), self._ptr(ws), ws.numel(), self._stream()))
        return wav

    # ------------------------------------------------------------------ token streams
    # Thin wrappers of dcx_stream_*: every tensor is the caller's, so a captured hipGraph keeps its
    # buffers (streaming.TokenStream owns them and mirrors the slots' counters on the host).
    def stream_state_size(self, sessions: int, push_frames: int, halo_frames: int) -> int:
        return int(self.L.dcx_stream_state_size(self.h, sessions, push_frames, halo_frames))

    def stream_state(self, sessions: int, push_frames: int, halo_frames: int) -> torch.Tensor:
        """A reset state buffer for `sessions` slots (dcx_stream_state_size, dcx_stream_reset)."""
        need = self.stream_state_size(sessions, push_frames, halo_frames)
        if need == 0:
            raise ValueError(f"token stream: bad geometry (sessions={sessions}, push_frames={push_frames}, "
                             f"halo_frames={halo_frames})")
        state = torch.empty(need, dtype=torch.uint8, device=self.device)
        self.stream_reset(state, sessions, push_frames, halo_frames)
        return state

    def stream_reset(self, state: torch.Tensor, sessions: int, push_frames: int, halo_frames: int) -> None:
        with torch.cuda.device(self.device):
            self._check(self.L.dcx_stream_reset(self.h, self._ptr(state), state.numel(), sessions, push_frames, halo_frames,
                                                self._stream()))

    def stream_step(self, state: torch.Tensor, sessions: int, push_frames: int, halo_frames: int, new_codes: torch.Tensor,
                    n_new: torch.Tensor, flags: torch.Tensor, wav_out: torch.Tensor, n_out: torch.Tensor,
                    n_invalid: torch.Tensor | None = None, ws: torch.Tensor | None = None) -> None:
        """One step of every slot (dcx_stream_decode_step) on the caller's device tensors: new_codes
        int32 (sessions, push_frames(, R)), n_new / flags / n_out int32 (sessions,), wav_out fp32
        (sessions, 256 (push_frames + halo_frames)), n_invalid int32 (1,) or None."""
        if not self.with_generator:
            raise RuntimeError("this engine was built without generator weights")
        B, P, h = sessions, push_frames, halo_frames
        want = {"new_codes": (new_codes, torch.int32, self._codes_shape(B, P)), "n_new": (n_new, torch.int32, (B,)),
                "flags": (flags, torch.int32, (B,)), "n_out": (n_out, torch.int32, (B,)),
                "wav_out": (wav_out, torch.float32, (B, self.hop * (P + h)))}
        if n_invalid is not None:
            want["n_invalid"] = (n_invalid, torch.int32, (1,))
        for name, (t, dtype, shape) in want.items():
            if t.device != self.device or t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous():
                raise ValueError(f"{name} must be a contiguous {dtype} tensor shaped {shape} on {self.device}")
        if ws is None:
            ws = self.workspace(B, P + 2 * h)
        elif ws.device != self.device or ws.dtype != torch.uint8 or not ws.is_contiguous():
            raise ValueError(f"workspace must be a contiguous uint8 tensor on {self.device}")
        with torch.cuda.device(self.device):  # the call itself checks the sizes of state and ws
            self._check(self.L.dcx_stream_decode_step(self.h, self._ptr(state), state.numel(), B, P, h, self._ptr(new_codes),
                                                      self._ptr(n_new), self._ptr(flags), self._ptr(wav_out),
                                                      self._ptr(n_out), self._ptr(n_invalid), self._ptr(ws), ws.numel(),
                                                      self._stream()))

    @staticmethod
    def stream_plan_step(halo_frames: int, push_frames: int, T: int, E: int, closed: int, n_new: int, flags: int):
        """dcx_stream_plan_step (host only): (T, E, closed, len, skip, take) after one step of a slot."""
        L = _native.lib()
        v = [ctypes.c_int32(x) for x in (T, E, closed, 0, 0, 0)]
        rc = L.dcx_stream_plan_step(halo_frames, push_frames, ctypes.byref(v[0]), ctypes.byref(v[1]), ctypes.byref(v[2]),
                                    n_new, flags, ctypes.byref(v[3]), ctypes.byref(v[4]), ctypes.byref(v[5]))
        if rc != _native.DCX_OK:
            raise ValueError("dcx_stream_plan_step: halo_frames must be >= 0 and push_frames >= 1")
        return tuple(x.value for x in v)

    # ------------------------------------------------------------------ audio streams
    # Thin wrappers of dcx_stream_encode_*, shaped like the token-stream ones (streaming.AudioStream
    # owns the tensors and mirrors the slots' counters on the host).
    def audio_stream_geometry(self, push_samples: int, halo_frames: int) -> tuple[int, int, int]:
        """(Ws, Wf, K) of a geometry: the window's samples and frames, the rows of a step's outputs."""
        v = [ctypes.c_int64(0) for _ in range(3)]
        if self.L.dcx_stream_encode_geometry(self.h, push_samples, halo_frames, *[ctypes.byref(x) for x in v]) != _native.DCX_OK:
            raise ValueError(f"audio stream: bad geometry (push_samples={push_samples}, halo_frames={halo_frames})")
        return tuple(x.value for x in v)

    def audio_stream_state_size(self, sessions: int, push_samples: int, halo_frames: int, want_pjt_in: bool = False) -> int:
        return int(self.L.dcx_stream_encode_state_size(self.h, sessions, push_samples, halo_frames, int(want_pjt_in)))

    def audio_stream_state(self, sessions: int, push_samples: int, halo_frames: int, want_pjt_in: bool = False) -> torch.Tensor:
        """A reset state buffer for `sessions` slots (dcx_stream_encode_state_size, dcx_stream_encode_reset)."""
        need = self.audio_stream_state_size(sessions, push_samples, halo_frames, want_pjt_in)
        if need == 0:
            raise ValueError(f"audio stream: bad geometry (sessions={sessions}, push_samples={push_samples}, "
                             f"halo_frames={halo_frames})")
        state = torch.empty(need, dtype=torch.uint8, device=self.device)
        self.audio_stream_reset(state, sessions, push_samples, halo_frames, want_pjt_in)
        return state

    def audio_stream_reset(self, state: torch.Tensor, sessions: int, push_samples: int, halo_frames: int,
                           want_pjt_in: bool = False) -> None:
        with torch.cuda.device(self.device):
            self._check(self.L.dcx_stream_encode_reset(self.h, self._ptr(state), state.numel(), sessions, push_samples,
                                                       halo_frames, int(want_pjt_in), self._stream()))

    def audio_stream_workspace_size(self, sessions: int, push_samples: int, halo_frames: int) -> int:
        Ws, _, _ = self.audio_stream_geometry(push_samples, halo_frames)
        return self.slots_workspace_size(sessions, Ws)

    def audio_stream_step(self, state: torch.Tensor, sessions: int, push_samples: int, halo_frames: int,
                          new_samples: torch.Tensor, n_new: torch.Tensor, flags: torch.Tensor, codes_out: torch.Tensor,
                          n_out: torch.Tensor, pjt_in_out: torch.Tensor | None = None, ws: torch.Tensor | None = None) -> None:
        """One step of every slot (dcx_stream_encode_step) on the caller's device tensors: new_samples
        fp32 (sessions, push_samples), n_new / flags / n_out int32 (sessions,), codes_out int32
        (sessions, K(, R)), pjt_in_out fp32 (sessions, K, codebook_dim) or None."""
        B, P, h = sessions, push_samples, halo_frames
        K = self.audio_stream_geometry(P, h)[2]
        want = {"new_samples": (new_samples, torch.float32, (B, P)), "n_new": (n_new, torch.int32, (B,)),
                "flags": (flags, torch.int32, (B,)), "n_out": (n_out, torch.int32, (B,)),
                "codes_out": (codes_out, torch.int32, self._codes_shape(B, K))}
        if pjt_in_out is not None:
            want["pjt_in_out"] = (pjt_in_out, torch.float32, (B, K, self.CD))
        for name, (t, dtype, shape) in want.items():
            if t.device != self.device or t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous():
                raise ValueError(f"{name} must be a contiguous {dtype} tensor shaped {shape} on {self.device}")
        if ws is None:
            ws = self._workspace_of(self.audio_stream_workspace_size(B, P, h), None)
        elif ws.device != self.device or ws.dtype != torch.uint8 or not ws.is_contiguous():
            raise ValueError(f"workspace must be a contiguous uint8 tensor on {self.device}")
        with torch.cuda.device(self.device):  # the call itself checks the sizes of state and ws
            self._check(self.L.dcx_stream_encode_step(self.h, self._ptr(state), state.numel(), B, P, h, self._ptr(new_samples),
                                                      self._ptr(n_new), self._ptr(flags), self._ptr(codes_out),
                                                      self._ptr(n_out), self._ptr(pjt_in_out), self._ptr(ws), ws.numel(),
                                                      self._stream()))

    def audio_stream_plan_step(self, halo_frames: int, push_samples: int, M: int, C: int, closed: int, n_new: int, flags: int):
        """dcx_stream_encode_plan_step (host only): (M, C, closed, len, start, skip, take) after one step
        of a slot."""
        v = [ctypes.c_int32(x) for x in (M, C, closed, 0, 0, 0, 0)]
        rc = self.L.dcx_stream_encode_plan_step(self.h, halo_frames, push_samples, ctypes.byref(v[0]), ctypes.byref(v[1]),
                                                ctypes.byref(v[2]), n_new, flags, *[ctypes.byref(x) for x in v[3:]])
        if rc != _native.DCX_OK:
            raise ValueError("dcx_stream_encode_plan_step: halo_frames must be >= 0 and push_samples >= 1")
        return tuple(x.value for x in v)

    def module_io(self, name: str) -> tuple[int, int, int]:
        """(input channels, output channels (0: int32 codes), output rows per input row) of a module."""
        ci, co, r = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        self._check(self.L.dcx_module_io(self.h, name.encode(), ctypes.byref(ci), ctypes.byref(co), ctypes.byref(r)))
        return ci.value, co.value, r.value

    def module_workspace_size(self, name: str, batch: int, rows: int) -> int:
        return int(self.L.dcx_module_workspace_size(self.h, name.encode(), batch, rows))

    def module(self, name: str, x: torch.Tensor, ws: torch.Tensor | None = None) -> torch.Tensor:
        """One reference module by its state-dict prefix (dcx_module_forward): x channels-last
        (B, L, C) fp32 -> y (see the header for shapes; int32 codes for "quantizer.search").
        ValueError for an unknown name or an input whose channel count is not the module's.
        ws: a caller-owned workspace of at least module_workspace_size bytes (the module's intermediate
        tensors, range maxima and shifts are laid out in it, in the same places for the same shapes)."""
        cin, cout, rate = self.module_io(name)
        x = self._dev(x, torch.float32)
        if x.ndim != 3 or x.shape[2] != cin:
            raise ValueError(f"{name} takes (B, L, {cin}) input, got {tuple(x.shape)}")
        B, L, C = x.shape
        n = name.encode()
        need = int(self.L.dcx_module_workspace_size(self.h, n, B, L))
        if need == 0:
            raise ValueError(f"module {name!r} cannot run on this handle")
        if cout == 0:  # "quantizer.search": layer 0's codes, one per row
            y = torch.empty(B, L, dtype=torch.int32, device=self.device)
        else:
            y = torch.empty(B, L * rate, cout, device=self.device)
        ws = torch.empty(need, dtype=torch.uint8, device=self.device) if ws is None else self._workspace_of(need, ws)
        with torch.cuda.device(self.device):
            self._check(self.L.dcx_module_forward(self.h, n, self._ptr(x), B, L, C, self._ptr(y), self._ptr(ws), ws.numel(),
                                                  self._stream()))
        return y

    def transpose(self, x: torch.Tensor) -> torch.Tensor:
        """(B, R, C) -> (B, C, R) contiguous, on device, by the HIP transpose kernel."""
        x = self._dev(x, torch.float32)
        B, R, C = x.shape
        out = torch.empty(B, C, R, device=self.device)
        with torch.cuda.device(self.device):
            rc = self.L.dcx_transpose(self._ptr(x), self._ptr(out), B, R, C, self._stream())
        if rc != _native.DCX_OK:
            raise _native.NativeError(rc, "dcx_transpose failed")
        return out

    # ------------------------------------------------------------------ profiling
    def profile(self, on: bool):
        self._check(self.L.dcx_profile_enable(self.h, 1 if on else 0))

    def vq_rescore_stats(self, reset: bool = False) -> tuple[int, int]:
        """(rows rescored, codes rescored) by the x6 VQ search since the last reset (synchronises)."""
        import ctypes
        r, c = ctypes.c_int64(0), ctypes.c_int64(0)
        self._check(self.L.dcx_vq_rescore_stats(self.h, ctypes.byref(r), ctypes.byref(c), int(reset)))
        return r.value, c.value

    def profile_reset(self):
        self._check(self.L.dcx_profile_reset(self.h))

    def profile_read(self) -> dict:
        out = {}
        n = self.L.dcx_profile_count(self.h)
        for i in range(n):
            name = ctypes.c_char_p()
            launches = ctypes.c_int64()
            ms, fl, by = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
            self._check(self.L.dcx_profile_read(self.h, i, ctypes.byref(name), ctypes.byref(launches), ctypes.byref(ms),
                                                ctypes.byref(fl), ctypes.byref(by)))
            out[name.value.decode()] = {"launches": launches.value, "ms": ms.value, "flops": fl.value, "bytes": by.value}
        return out


class NativeConv:
    """The conv primitive of libdcx (dcx_conv_*): Conv1d ("same" padding, dilation) or
    ConvTranspose1d (padding (k-stride)/2) on channels-last fp32 tensors.  h3=True: in gemm="x6", convs
    the stages would run in h3 arithmetic take the h3 kernels (dcx_conv_set_h3); last_kernel names the
    kernel the last call launched."""

    def __init__(self, weight: np.ndarray, bias=None, dilation: int = 1, transposed: bool = False, stride: int = 1,
                 h3: bool = False):
        self.L = _native.lib()
        w = np.ascontiguousarray(weight, dtype=np.float32)
        if transposed:
            self.cin, self.cout, self.k = w.shape
        else:
            self.cout, self.cin, self.k = w.shape
        b = None if bias is None else np.ascontiguousarray(bias, dtype=np.float32)
        self.stride = stride if transposed else 1
        self._b = b
        h = ctypes.c_void_p()
        rc = self.L.dcx_conv_create(w.ctypes.data_as(ctypes.c_void_p), None if b is None else b.ctypes.data_as(ctypes.c_void_p),
                                    self.cin, self.cout, self.k, dilation, 1 if transposed else 0, stride, ctypes.byref(h))
        if rc != _native.DCX_OK:
            raise ValueError(f"dcx_conv_create failed: {self.L.dcx_status_string(rc).decode()}")
        self.h = h
        if h3 and self.L.dcx_conv_set_h3(self.h, 1) != _native.DCX_OK:
            raise ValueError("dcx_conv_set_h3 failed")

    def set_knob(self, name: str, value: int):
        """An A/B switch of the primitive's own handle (dcx_conv_set_knob), e.g. DCX_H3_BN."""
        rc = self.L.dcx_conv_set_knob(self.h, name.encode(), int(value))
        if rc != _native.DCX_OK:
            raise _native.NativeError(rc, f"dcx_conv_set_knob({name}) failed")

    @property
    def last_kernel(self) -> str:
        return self.L.dcx_conv_last_kernel(self.h).decode()

    def __del__(self):
        h = getattr(self, "h", None)
        if h:
            self.L.dcx_conv_destroy(h)
            self.h = None

    def __call__(self, x: torch.Tensor, gemm: str = "x6", epi: int = 0, res: torch.Tensor | None = None,
                 want_y: bool = True, want_silu: bool = False):
        B, Lin, C = x.shape
        assert C == self.cin and x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()
        Lout = Lin * self.stride
        y = torch.empty(B, Lout, self.cout, device=x.device) if want_y else None
        ys = torch.empty(B, Lout, self.cout, device=x.device) if want_silu else None
        ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
        rc = self.L.dcx_conv_forward(self.h, GEMM_MODES[gemm], ptr(x), B, Lin, ptr(y), ptr(ys), ptr(res), epi,
                                     ctypes.c_void_p(torch.cuda.current_stream(x.device).cuda_stream))
        if rc != _native.DCX_OK:
            raise _native.NativeError(rc, "dcx_conv_forward failed")
        return (y, ys) if want_silu else y

    def forward_h3(self, x: torch.Tensor, want_y: bool = False, want_silu: bool = False, want_silu_h2: bool = False,
                   want_amax: bool = False, res: torch.Tensor | None = None, in_place: bool = False,
                   macc: torch.Tensor | None = None, mean: int = 0, lens: torch.Tensor | None = None) -> dict:
        """A tap conv in h3 arithmetic with the outputs a generator stage asks for (dcx_conv_forward_h3):
        fp32 y / silu, the silu image in h2 (int16 words) with its per-clip shifts, the measured per-clip
        max |v|; res: v = res + conv (in_place: y is res itself); mean 1 / 2 / 3 on macc (updated in
        place); lens: int32 per-clip row counts.  Returns the requested tensors by name."""
        B, L, C = x.shape
        assert C == self.cin and x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and self.stride == 1
        dev = x.device
        out = {}
        if want_y:
            out["y"] = res if in_place else torch.empty(B, L, self.cout, device=dev)
        if want_silu:
            out["y_silu"] = torch.empty(B, L, self.cout, device=dev)
        if want_silu_h2:
            out["y_silu_h2"] = torch.zeros(B, L, self.cout * 2, dtype=torch.int16, device=dev)
            out["y_ash"] = torch.zeros(B, dtype=torch.int32, device=dev)
        if want_amax:
            out["y_amax"] = torch.zeros(B, device=dev)
        keep = [res.abs().amax(dim=(1, 2)).contiguous() if res is not None else None,
                macc.abs().amax(dim=(1, 2)).contiguous() if macc is not None and mean >= 2 else None]
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        o = _native.ConvH3Out(ptr(out.get("y")), ptr(out.get("y_silu")), ptr(out.get("y_silu_h2")), ptr(out.get("y_ash")),
                              ptr(out.get("y_amax")), ptr(res), ptr(keep[0]), ptr(macc), ptr(keep[1]), ptr(lens),
                              3 if res is not None else 0, mean)
        rc = self.L.dcx_conv_forward_h3(self.h, ctypes.c_void_p(x.data_ptr()), B, L, ctypes.byref(o),
                                        ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        if rc != _native.DCX_OK:
            raise _native.NativeError(rc, "dcx_conv_forward_h3 failed")
        if macc is not None:
            out["macc"] = macc
        return out
