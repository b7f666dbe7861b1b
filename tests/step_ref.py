"""TEST INFRA: the dropout masks of one whole engine forward, for the mask-injecting
oracle (oracle/model_ref.py, `masks`), with no GPU dependency.  tests/test_step_ref.py
proves the reference they make; tests/test_dropout_step_parity_gpu.py judges a whole
training step by it.  Never imported by the package.

Nothing here restates the hash.  A site's seed is engine._seed(base, is_encoder, layer,
site); its keep decisions come from the restatement that already judges the kernel
writing that site, and so does its scale:
  resid, drop1, xresid, drop2x, drop2, drop3   rowwise_ref.keep_pattern on [B*T][D]
      (the LayerNorm tail, norm.hip; scale 1 / (1 - p) per mask: rowwise_ref.branch_mask)
  ffn                                          gemm_ref.keep_flat on [B*T][4D]
      (the FFN1 epilogue; scale gemm_ref.inv_keep(p))
  attn, xattn                                  attn_ref.keep on [B*H][T][T]
      (scale gemm_ref.inv_keep(p): attn_ref._keep_factor)"""
import torch

from neurosync_trainer_lite_amd.engine import _SITE, _seed
from tests import attn_ref as A
from tests import gemm_ref as G
from tests import rowwise_ref as R

ENC_SITES = ("attn", "resid", "drop1", "ffn", "drop2")
DEC_SITES = ("attn", "resid", "drop1", "xattn", "xresid", "drop2x", "ffn", "drop3")
LN_SITES = ("resid", "drop1", "xresid", "drop2x", "drop2", "drop3")
assert set(ENC_SITES) | set(DEC_SITES) == set(_SITE)


def salted_seed(draw, seed_salt):
    """engine.Seq2SeqEngine.draw_seed's formula on a given torch draw (p > 0)."""
    return (draw + seed_salt * 0x9E3779B97F4A7C15) % (1 << 62)


def site_keep(seed, site, B, T, D, H, p):
    """bool tensor of one site's keep decisions, shaped like the tensor it masks."""
    if site in ("attn", "xattn"):
        return torch.from_numpy(A.keep(seed, B * H, T, p)).reshape(B, H, T, T)
    if site == "ffn":
        return torch.from_numpy(G.keep_flat(seed, B * T, 4 * D, p)).reshape(B, T, 4 * D)
    return torch.from_numpy(R.keep_pattern(seed, B * T, D, p)).reshape(B, T, D)


def site_scale(site, p):
    if site in LN_SITES:
        return R.branch_mask(1, 2, 1, p, (0,))[1]
    return G.inv_keep(p)


def site_keys(L):
    return [(enc, l, s) for enc, sites in ((True, ENC_SITES), (False, DEC_SITES)) for l in range(L) for s in sites]


def site_masks(base_seed, B, T, D, H, L, p, dtype=torch.float64):
    """{(is_encoder, layer, site): keep / (1 - p)} of a forward whose base seed
    (engine.saved["seed"]) is base_seed."""
    return {(enc, l, s): site_keep(_seed(base_seed, enc, l, s), s, B, T, D, H, p).to(dtype) * site_scale(s, p)
            for enc, l, s in site_keys(L)}
