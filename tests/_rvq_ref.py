"""The residual chain of DownsampleGRVQ with n_codebooks > 1 (residual_vq.py:140-259) in plain torch,
for the tests of the native path:

    r_0 = x_pjt_in;  c_k = argmin_j |r_k - E_k[j]|^2 (fp64, first index on ties);
    r_{k+1} = fl32(r_k - E_k[c_k]);  quantized_fup = fl32(((E_0[c_0] + E_1[c_1]) + ...) + E_{R-1}[c_{R-1}])

`tests/test_rvq_host.py` pins it to the reference's own outputs (tests/golden/rvq.npz): the codes and
quantized_fup bit for bit.  Everything runs on the device of its inputs (the CPU, or the GPU in
tests/test_gpu_rvq.py).
"""
from __future__ import annotations

import copy

import numpy as np
import torch
import torch.nn.functional as F

FIXTURE_SEED = 1234
FEAT_SEED = 77
FEAT_SHAPE = (2, 1024, 45)
DECISIVE_GAP = 1e-4  # tests/_parity.py's threshold


def rvq_cfg(codebook_size: int = 4096, codebook_dim: int = 256, n_codebooks: int = 3) -> dict:
    """The default configuration with another quantizer geometry."""
    from distilcodec_nabeel_amd import config

    cfg = copy.deepcopy(config.default_config())
    cfg["quantizer"].update(n_codebooks=n_codebooks, codebook_size=codebook_size, codebook_dim=codebook_dim)
    return cfg


def fixture_feat() -> torch.Tensor:
    """The fixture's input (B, 1024, T): seeded, so it is not stored."""
    return torch.randn(*FEAT_SHAPE, generator=torch.Generator().manual_seed(FEAT_SEED)) * 0.5


def masked_codes(codes_btr: np.ndarray) -> np.ndarray:
    """The fixture's masked decode input: layer 1 masked on clip 0 frames 3-7, a whole frame on clip 1."""
    c = np.array(codes_btr, dtype=np.int64, copy=True)
    c[0, 3:8, 1] = -1
    c[1, 0, :] = -1
    return c


def codebooks(sd_q: dict, R: int, device="cpu") -> list:
    return [torch.as_tensor(np.asarray(sd_q[f"grvq.rvqs.0.layers.{k}._codebook.embed"]))[0].to(device) for k in range(R)]


def argmin_top2_fp64(x: torch.Tensor, E: torch.Tensor, chunk: int = 512):
    """(first index of the fp64 minimum of |x - E_j|^2 per row, relative gap of the two smallest).
    Distances within 1e-12 relative of the minimum count as ties (tests/test_gpu_vq.py's rule)."""
    E64 = E.to(torch.float64)
    e2 = (E64 ** 2).sum(1)
    idx, gap = [], []
    for s in range(0, x.shape[0], chunk):
        x64 = x[s: s + chunk].to(torch.float64)
        d = (x64 ** 2).sum(1)[:, None] + e2[None, :] - 2.0 * (x64 @ E64.T)
        m = d.min(dim=1, keepdim=True).values
        tie = d <= m + 1e-12 * m.abs()
        idx.append(torch.argmax(tie.to(torch.int8), dim=1))
        two = torch.topk(d, 2, dim=1, largest=False).values
        gap.append((two[:, 1] - two[:, 0]) / two[:, 1].abs().clamp_min(1e-300))
    return torch.cat(idx), torch.cat(gap)


def chain(x_pjt_in: torch.Tensor, Es: list):
    """x_pjt_in (rows, CD) fp32 -> (codes (rows, R) int64, quantized_fup (rows, CD) fp32, decisive
    (rows, R) bool: the top-2 gap exceeds DECISIVE_GAP at every layer <= k)."""
    r = x_pjt_in.to(torch.float32)
    codes, fup, ok = [], None, torch.ones(r.shape[0], dtype=torch.bool, device=r.device)
    decisive = []
    for E in Es:
        c, gap = argmin_top2_fp64(r, E)
        ok = ok & (gap > DECISIVE_GAP)
        q = E[c]
        r = r - q
        fup = q if fup is None else fup + q
        codes.append(c)
        decisive.append(ok)
    return torch.stack(codes, 1), fup, torch.stack(decisive, 1)


def _lin(sd_q, name, x):
    return F.linear(x, torch.as_tensor(sd_q[f"{name}.weight"]).to(x), torch.as_tensor(sd_q[f"{name}.bias"]).to(x))


def project_in(feat: torch.Tensor, sd_q: dict) -> torch.Tensor:
    """feat (B, D, T) -> x_pjt_in (B, T, CD): down conv + ConvNeXt block + project_in (grfvq.py:105-116)."""
    from oracle import reference_cpu as R

    x = F.conv1d(feat, R._t(sd_q, "downsample.0.0.weight", torch.float32), R._t(sd_q, "downsample.0.0.bias", torch.float32))
    x = R.convnext_block(x, sd_q, "downsample.0.1", torch.float32)
    return _lin(sd_q, "grvq.rvqs.0.project_in", x.mT)


def upsampled(q_sum: torch.Tensor, sd_q: dict) -> torch.Tensor:
    """sum of the layers' rows (B, T, CD) -> (B, D, T): project_out + up ConvT + ConvNeXt block."""
    from oracle import reference_cpu as R

    return R._vq_upsample(_lin(sd_q, "grvq.rvqs.0.project_out", q_sum).mT, sd_q, torch.float32)


def forward(feat: torch.Tensor, sd_q: dict, R: int) -> dict:
    """DownsampleGRVQ.forward in eval mode on the CPU: codes (B, T, R), x_pjt_in, quantized_fup
    (B, T, CD), quantized (B, D, T), decisive (B, T, R)."""
    pin = project_in(feat, sd_q)
    B, T, CD = pin.shape
    codes, fup, dec = chain(pin.reshape(-1, CD), codebooks(sd_q, R))
    fup = fup.reshape(B, T, CD)
    return {"codes": codes.reshape(B, T, R), "x_pjt_in": pin, "quantized_fup": fup, "quantized": upsampled(fup, sd_q),
            "decisive": dec.reshape(B, T, R)}


def gather_sum(codes_btr: torch.Tensor, Es: list) -> torch.Tensor:
    """sum_k masked(E_k[c_k]) in fp32, in layer order (residual_vq.py:103-138): -1 adds nothing,
    other negative codes wrap."""
    out = None
    for k, E in enumerate(Es):
        c = codes_btr[..., k].long()
        m = c == -1
        q = E[c.masked_fill(m, 0)].masked_fill(m[..., None], 0.0)
        out = q if out is None else out + q
    return out


def decode(codes_btr: torch.Tensor, sd_q: dict) -> torch.Tensor:
    """DownsampleGRVQ.decode of (B, T, R) codes -> z (B, D, T)."""
    R = codes_btr.shape[-1]
    return upsampled(gather_sum(torch.as_tensor(codes_btr), codebooks(sd_q, R)), sd_q)
