"""Fixture of the residual-VQ tests: the reference's own DownsampleGRVQ with three codebooks.

Run where the reference checkout is available (tests/golden/_ref_loader.py); writes
tests/golden/rvq.npz.  The model is the reference's DownsampleGRVQ(input_dim 1024, n_codebooks 3,
codebook_size 4096, codebook_dim 256, downsample_factor [1]) in eval mode on the CPU with the
weights of `weights.synthetic_quantizer(rvq_cfg(), seed=1234)`; the input is the seeded
`_rvq_ref.fixture_feat()` (not stored).  Stored: forward's codes (B, T, R), x_pjt_in,
quantized_fup, quantized; encode()'s indices (B, R, T); decode() of `_rvq_ref.masked_codes(codes)`.

The generator asserts what tests/test_rvq_host.py asserts again on the stored file: the chain of
tests/_rvq_ref.py reproduces the reference's codes and quantized_fup bit for bit, and at least 90 %
of the (frame, layer) entries are decisive.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import _rvq_ref as RV  # noqa: E402
from distilcodec_nabeel_amd import weights  # noqa: E402


def main():
    import _ref_loader

    _ref_loader.import_reference()
    from distilcodec.vector_quantization.grfvq import DownsampleGRVQ

    torch.manual_seed(0)
    torch.set_num_threads(1)
    cfg = RV.rvq_cfg()
    q = cfg["quantizer"]
    R = q["n_codebooks"]
    mod = DownsampleGRVQ(input_dim=q["input_dim"], n_codebooks=R, n_groups=1, codebook_size=q["codebook_size"],
                         codebook_dim=q["codebook_dim"], downsample_factor=[1])
    sd = weights.synthetic_quantizer(cfg, seed=RV.FIXTURE_SEED)
    missing, unexpected = mod.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    assert not unexpected, unexpected
    assert all(m.endswith(("_codebook.embed_avg", "_codebook.cluster_size")) for m in missing), missing
    mod.eval()
    feat = RV.fixture_feat()
    with torch.no_grad():
        ret = mod(feat)
        codes = ret.codes[0]  # (G=1, B, T, R)
        enc = mod.encode(feat)
        masked = RV.masked_codes(codes.numpy())
        z_masked = mod.decode(torch.from_numpy(masked)[None])
    ours = RV.forward(feat, sd, R)
    assert torch.equal(ours["codes"], codes), "the torch chain does not reproduce the reference's codes"
    assert torch.equal(ours["quantized_fup"], ret.quantized_fup.reshape(ours["quantized_fup"].shape))
    share = ours["decisive"].float().mean(dim=(0, 1)).tolist()
    print("decisive share per layer:", share)
    assert min(share) >= 0.9, share
    out = {
        "codes": codes.numpy().astype(np.int32),
        "x_pjt_in": ret.x_pjt_in.reshape(ours["x_pjt_in"].shape).numpy(),
        "quantized_fup": ret.quantized_fup.reshape(ours["quantized_fup"].shape).numpy(),
        "quantized": ret.quantized.numpy(),
        "encode": enc.numpy().astype(np.int32),
        "masked_codes": masked.astype(np.int32),
        "z_masked": z_masked.numpy(),
    }
    path = os.path.join(HERE, "rvq.npz")
    np.savez(path, **out)
    print(path, os.path.getsize(path), "bytes", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
