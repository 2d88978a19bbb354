"""MI355X-native Florence-2 icon captioner: DaViT vision tower + projector + BART encoder + on-device
greedy decoder, as three static plans (vision+encoder, cross-KV, one decoder step) replayed from HIP
graphs.  Replaces, for `icon_caption`, what the reference reaches through
`processor(...)` + `model.generate(...)` (ref:util/utils.py:116-130) — i.e. transformers' Florence-2
(hf:models/florence2/modeling_florence2.py), BART (hf:models/bart/modeling_bart.py) and the greedy
loop of hf:generation/utils.py:2783-2937.  Host Python only wires pointers; there is no torch math
on the path and no CPU fallback.
"""
import contextlib
import json
import math
import os
from pathlib import Path
from types import SimpleNamespace
from typing import Dict, List, Optional

import numpy as np
import torch

from . import _lib as L
from .planner import PlanBuilder, View, torch_dtype

PROMPT_IDS = [0, 2264, 473, 5, 2274, 6190, 116, 2]   # <s>What does the image describe?</s>  
# Text capacities of a plan whose prompt is an INPUT (ids + per-row key counts, see `_CaptionPlans`): a prompt runs on the smallest
# capacity that holds it.  The ladder is short on purpose: every capacity is one more set of resident plans (several GB each at
# 768x768 crops), and the encoder computes the padded positions.  The default prompt needs none of this (capacity 8, a constant block).
TEXT_CAPACITIES = (8, 16, 32, 64)


def text_capacity(n_tokens: int) -> int:
    """smallest text capacity of a plan that holds a prompt of n_tokens ids; more than 64 tokens is a ValueError"""
    for c in TEXT_CAPACITIES:
        if n_tokens <= c:
            return c
    raise ValueError(f"a prompt of {n_tokens} tokens exceeds the captioner's limit of {TEXT_CAPACITIES[-1]} prompt tokens "
                     "(bos and eos included)")


_BUCKETS = tuple(sorted({min(max(int(x), 1), 128) for x in os.environ.get("OMNI_CAPTION_BUCKETS", "8,16,32,64,96,128").split(",")} | {128}))
CLIP_MEAN = (0.485, 0.456, 0.406)
CLIP_STD = (0.229, 0.224, 0.225)


# ------------------------------------------------------------------------------------------ weights
def _legacy_to_native(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """Map the remote-code (`trust_remote_code`) Florence-2 key names to the native transformers ones
    (from memory — audited only against the native layout, no legacy checkpoint here)."""
    out = {}
    for k, v in sd.items():
        nk = k
        if nk.startswith("vision_tower."):
            nk = nk.replace(".proj.", ".conv.") if ".convs." in nk else nk
            nk = nk.replace(".fn.dw.", ".")
            nk = nk.replace(".window_attn.norm.", ".norm1.").replace(".channel_attn.norm.", ".norm1.")
            nk = nk.replace(".window_attn.fn.", ".window_attn.").replace(".channel_attn.fn.", ".channel_attn.")
            nk = nk.replace(".ffn.norm.", ".norm2.").replace(".ffn.fn.net.", ".ffn.")
            nk = "model." + nk
        elif nk == "image_projection":
            nk, v = "model.multi_modal_projector.image_projection.weight", v.t().contiguous()
        elif nk.startswith("image_proj_norm."):
            nk = "model.multi_modal_projector." + nk
        elif nk.startswith("image_pos_embed."):
            nk = "model.multi_modal_projector.image_position_embed." + nk[len("image_pos_embed."):]
        elif nk.startswith("visual_temporal_embed."):
            nk = "model.multi_modal_projector." + nk
        elif nk.startswith("language_model.model."):
            nk = "model.language_model." + nk[len("language_model.model."):]
        elif nk == "language_model.lm_head.weight":
            nk = "lm_head.weight"
        elif nk == "language_model.final_logits_bias":
            nk = "final_logits_bias"
        out[nk] = v
    return out


def normalise_config(cfg: dict) -> dict:
    """config.json of the remote-code (`trust_remote_code`) Florence-2 — what the reference actually loads (ref:util/utils.py:63-68,
    weights/icon_caption_florence/config.json) — in the vocabulary of the native transformers config this module reads: the DaViT
    widths are `dim_embed` there (`embed_dim` natively), the learned 2-D position table and the temporal table carry their sizes in
    nested dicts (`image_pos_embed.max_pos_embeddings`, `visual_temporal_embedding.max_temporal_embeddings`), and the generation
    defaults (`no_repeat_ngram_size`, `forced_bos_token_id`, ...) sit in `text_config` or at the top level.  Returns a copy; a native
    config passes through unchanged.  A config that names neither spelling raises a ValueError that says which key is missing —
    never a bare KeyError from deep inside the loader."""
    cfg = json.loads(json.dumps(cfg))
    vc = cfg.get("vision_config")
    tc = cfg.get("text_config")
    if not isinstance(vc, dict) or not isinstance(tc, dict):
        raise ValueError("Florence-2 config.json needs `vision_config` and `text_config` objects")
    if "embed_dim" not in vc and "dim_embed" in vc:
        vc["embed_dim"] = list(vc["dim_embed"])
    pe = vc.get("image_pos_embed")
    if isinstance(pe, dict) and "max_position_embeddings" not in vc and "max_pos_embeddings" in pe:
        vc["max_position_embeddings"] = int(pe["max_pos_embeddings"])
    te = vc.get("visual_temporal_embedding")
    if isinstance(te, dict) and "max_temporal_embeddings" not in vc and "max_temporal_embeddings" in te:
        vc["max_temporal_embeddings"] = int(te["max_temporal_embeddings"])
    need_v = ("embed_dim", "depths", "num_heads", "num_groups", "patch_size", "patch_stride", "patch_padding", "patch_prenorm", "window_size",
              "projection_dim")
    need_t = ("d_model", "vocab_size", "encoder_layers", "decoder_layers", "encoder_attention_heads", "encoder_ffn_dim", "decoder_ffn_dim",
              "max_position_embeddings")
    missing = [f"vision_config.{k}" for k in need_v if k not in vc] + [f"text_config.{k}" for k in need_t if k not in tc]
    if missing:
        raise ValueError("Florence-2 config.json lacks " + ", ".join(missing) + " (native transformers names; the remote-code spellings "
                         "dim_embed / image_pos_embed / visual_temporal_embedding are translated)")
    return cfg


def expected_native_keys(cfg: dict) -> Dict[str, tuple]:
    """Every tensor a Florence-2 checkpoint in the native transformers layout must hold, with its shape, derived from config.json alone
    (hf:models/florence2/modeling_florence2.py module tree).  `FlorenceWeights` audits a checkpoint against it at load:
    a missing, unexpected or mis-shaped tensor is an error that names the offenders — never a silently random layer."""
    vc, tc = cfg["vision_config"], cfg["text_config"]
    dims, depths = vc["embed_dim"], vc["depths"]
    ratio = vc.get("mlp_ratio", 4.0)
    out = {}
    vt = "model.vision_tower."
    cin = vc.get("in_channels", 3)
    for i, C in enumerate(dims):
        k = vc["patch_size"][i]
        out[f"{vt}convs.{i}.conv.weight"] = (C, cin, k, k)
        out[f"{vt}convs.{i}.conv.bias"] = (C,)
        nd = cin if vc["patch_prenorm"][i] else C
        out[f"{vt}convs.{i}.norm.weight"] = out[f"{vt}convs.{i}.norm.bias"] = (nd,)
        hid = int(C * ratio)
        for j in range(depths[i]):
            for blk, attn in (("spatial_block", "window_attn"), ("channel_block", "channel_attn")):
                b = f"{vt}blocks.{i}.{j}.{blk}."
                for cv in ("conv1", "conv2"):
                    out[b + cv + ".weight"] = (C, 1, 3, 3)
                    out[b + cv + ".bias"] = (C,)
                for nm in ("norm1", "norm2"):
                    out[b + nm + ".weight"] = out[b + nm + ".bias"] = (C,)
                out[b + attn + ".qkv.weight"] = (3 * C, C)
                out[b + attn + ".qkv.bias"] = (3 * C,)
                out[b + attn + ".proj.weight"] = (C, C)
                out[b + attn + ".proj.bias"] = (C,)
                out[b + "ffn.fc1.weight"] = (hid, C)
                out[b + "ffn.fc1.bias"] = (hid,)
                out[b + "ffn.fc2.weight"] = (C, hid)
                out[b + "ffn.fc2.bias"] = (C,)
        cin = C
    mp = "model.multi_modal_projector."
    P, D = vc["projection_dim"], tc["d_model"]
    out[mp + "image_projection.weight"] = (P, dims[-1])
    out[mp + "image_proj_norm.weight"] = out[mp + "image_proj_norm.bias"] = (P,)
    out[mp + "image_position_embed.row_embeddings.weight"] = out[mp + "image_position_embed.column_embeddings.weight"] = \
        (vc.get("max_position_embeddings", 50), dims[-1] // 2)
    out[mp + "visual_temporal_embed.pos_idx_to_embed"] = (vc.get("max_temporal_embeddings", 100), dims[-1])
    lm = "model.language_model."
    out[lm + "shared.weight"] = (tc["vocab_size"], D)
    for side, n_layers, ffn in (("encoder", tc["encoder_layers"], tc["encoder_ffn_dim"]), ("decoder", tc["decoder_layers"], tc["decoder_ffn_dim"])):
        out[f"{lm}{side}.embed_positions.weight"] = (tc["max_position_embeddings"] + 2, D)
        out[f"{lm}{side}.layernorm_embedding.weight"] = out[f"{lm}{side}.layernorm_embedding.bias"] = (D,)
        for l in range(n_layers):
            b = f"{lm}{side}.layers.{l}."
            attns = ("self_attn",) if side == "encoder" else ("self_attn", "encoder_attn")
            for a in attns:
                for pj in ("q_proj", "k_proj", "v_proj", "out_proj"):
                    out[b + f"{a}.{pj}.weight"] = (D, D)
                    out[b + f"{a}.{pj}.bias"] = (D,)
                out[b + f"{a}_layer_norm.weight"] = out[b + f"{a}_layer_norm.bias"] = (D,)
            out[b + "fc1.weight"] = (ffn, D); out[b + "fc1.bias"] = (ffn,)
            out[b + "fc2.weight"] = (D, ffn); out[b + "fc2.bias"] = (D,)
            out[b + "final_layer_norm.weight"] = out[b + "final_layer_norm.bias"] = (D,)
    return out


# tensors a checkpoint MAY carry beyond the list above: the tied output embedding, the (all-zero) logits bias, the encoder / decoder
# copies of the shared embedding that older exports duplicate
_OPTIONAL_KEYS = {"lm_head.weight": lambda cfg: (cfg["text_config"]["vocab_size"], cfg["text_config"]["d_model"]),
                  "final_logits_bias": lambda cfg: (1, cfg["text_config"]["vocab_size"]),
                  "model.language_model.encoder.embed_tokens.weight": lambda cfg: (cfg["text_config"]["vocab_size"], cfg["text_config"]["d_model"]),
                  "model.language_model.decoder.embed_tokens.weight": lambda cfg: (cfg["text_config"]["vocab_size"], cfg["text_config"]["d_model"])}


def audit_checkpoint(sd: Dict[str, torch.Tensor], cfg: dict) -> None:
    """Strict audit of a (native-layout) state dict against config.json: raises ValueError naming what is wrong."""
    want = expected_native_keys(cfg)
    missing = sorted(k for k in want if k not in sd)
    unexpected = sorted(k for k in sd if k not in want and k not in _OPTIONAL_KEYS)
    shapes = sorted(f"{k}: {tuple(sd[k].shape)} != {want[k]}" for k in want if k in sd and tuple(sd[k].shape) != tuple(want[k]))
    shapes += sorted(f"{k}: {tuple(sd[k].shape)} != {_OPTIONAL_KEYS[k](cfg)}" for k in _OPTIONAL_KEYS
                     if k in sd and tuple(sd[k].shape) != tuple(_OPTIONAL_KEYS[k](cfg)))
    if missing or unexpected or shapes:
        show = lambda l: ", ".join(l[:6]) + (f" ... (+{len(l) - 6})" if len(l) > 6 else "")
        raise ValueError("Florence-2 checkpoint does not match its config.json: "
                         + "; ".join(p for p in (f"{len(missing)} missing [{show(missing)}]" if missing else "",
                                                 f"{len(unexpected)} unexpected [{show(unexpected)}]" if unexpected else "",
                                                 f"{len(shapes)} mis-shaped [{show(shapes)}]" if shapes else "") if p))


class FlorenceWeights:
    def __init__(self, model_dir):
        from safetensors.torch import load_file
        d = Path(model_dir)
        self.dir = d
        self.cfg = normalise_config(json.loads((d / "config.json").read_text()))
        gpath = d / "generation_config.json"
        self.gen = json.loads(gpath.read_text()) if gpath.exists() else {}
        files = sorted(d.glob("*.safetensors"))
        if not files:
            raise FileNotFoundError(f"no .safetensors under {d}")
        sd = {}
        for f in files:
            sd.update(load_file(str(f)))
        if any(k.startswith("vision_tower.") for k in sd):
            sd = _legacy_to_native(sd)
        audit_checkpoint(sd, self.cfg)           # strict: every tensor the config implies, with its shape, nothing unknown
        self.sd = {k: v.float() for k, v in sd.items()}
        if "lm_head.weight" not in self.sd:
            self.sd["lm_head.weight"] = self.sd["model.language_model.shared.weight"]
        vc, tc = self.cfg["vision_config"], self.cfg["text_config"]
        self.embed_dim = vc["embed_dim"]; self.depths = vc["depths"]; self.heads = vc["num_heads"]
        self.groups = vc["num_groups"]; self.patch = list(zip(vc["patch_size"], vc["patch_stride"], vc["patch_padding"]))
        self.prenorm = vc["patch_prenorm"]; self.window = vc["window_size"]
        self.d_model = tc["d_model"]; self.n_heads = tc["encoder_attention_heads"]
        self.enc_layers, self.dec_layers = tc["encoder_layers"], tc["decoder_layers"]
        self.vocab = self.sd["lm_head.weight"].shape[0]
        self.embed_scale = math.sqrt(self.d_model) if tc.get("scale_embedding", False) else 1.0
        # generation defaults: generation_config.json, else text_config, else the top level of config.json (where the remote-code config and
        # `_from_model_config` exports keep them), else the transformers default (no n-gram ban, nothing forced)
        g = lambda k, dflt: self.gen.get(k, tc.get(k, self.cfg.get(k, dflt)))
        self.pad, self.bos, self.eos = g("pad_token_id", 1), g("bos_token_id", 0), g("eos_token_id", 2)
        self.start = g("decoder_start_token_id", 2)
        self.ngram = g("no_repeat_ngram_size", 0) or 0
        fb, fe = g("forced_bos_token_id", None), g("forced_eos_token_id", None)
        self.forced_bos = -1 if fb is None else fb
        self.forced_eos = -1 if fe is None else fe
        # beam search (Florence2Captioner.generate(num_beams > 1)): transformers' defaults
        self.length_penalty = float(g("length_penalty", 1.0))
        self.early_stopping = check_early_stopping(g("early_stopping", False))
        assert self.window == 12 and self.d_model // self.n_heads == 64


def check_early_stopping(v):
    """transformers' `early_stopping`: True, False or "never" (anything else is an error, as there)."""
    if v is True or v is False or v == "never":
        return v
    raise ValueError(f"early_stopping must be True, False or 'never' (got {v!r})")


BEAM_MAX = 8                       # include/omni_amd.h OMNI_OP_BEAM_STEP: 2 <= k <= 8
BEAM_STAGING_BYTES = 48 * 1024     # OMNI_OP_BEAM_STEP stages 3 x k x T i32 / f32 positions in LDS


def beam_max_new(k: int) -> int:
    """largest max_new_tokens whose T = max_new_tokens + 1 positions of k beams fit the staging LDS of OMNI_OP_BEAM_STEP"""
    return BEAM_STAGING_BYTES // (3 * 4 * int(k)) - 1
_EARLY_STOPPING_CODE = {False: 0, True: 1, "never": 2}


def caption_confidence(ids_row, logp_row, eos, forced_bos, forced_eos, max_new):
    """Confidence of one greedy caption in (0, 1]: exp of the mean token log-probability — the geometric mean of the probabilities
    the model gave the tokens it chose — over the generated positions up to and including the first EOS (all of them when there is
    none).  ids_row: the sequence with the decoder start token at position 0; logp_row: aligned with ids_row[1:]
    (`generate(output_scores=True).token_logprobs`, `caption_crops(return_scores=True)`); further entries of either are ignored.
    Forced positions say nothing about the model and are left out: position 1 when forced_bos >= 0, position max_new when
    forced_eos >= 0.  None when no unforced position remains.  The single host definition (ScreenParser, get_som_labeled_img)."""
    ids = [int(t) for t in ids_row]
    lps = [float(v) for v in logp_row]
    n = min(len(ids) - 1, len(lps), int(max_new))
    vals = []
    for p in range(1, n + 1):
        forced = (forced_bos >= 0 and p == 1) or (forced_eos >= 0 and p == max_new)
        if not forced:
            vals.append(lps[p - 1])
        if ids[p] == eos:
            break
    if not vals:
        return None
    return float(math.exp(sum(vals) / len(vals)))


# ---- generation controls (OMNI_OP_GREEDY_CTRL_STEP): the ONE Python mirror of the control block of include/omni_amd.h
GEN_CTRL_KEYS = ("repetition_penalty", "no_repeat_ngram_size", "min_new_tokens", "suppress_tokens", "begin_suppress_tokens",
                 "bad_words_ids")
GEN_CTRL_HEADER_WORDS = 8          # struct omni_gen_ctrl: f32 penalty | i32 ngram | min_new_tokens | begin_index | n_bad | bad_stride | 0 | 0
GEN_CTRL_MAX_BAD = 64              # OMNI_GEN_CTRL_MAX_BAD: multi-token bad-word sequences
GEN_CTRL_MAX_BAD_LEN = 8           # OMNI_GEN_CTRL_MAX_BAD_LEN: tokens per sequence


def gen_ctrl_words(vocab: int, n_bad: int = GEN_CTRL_MAX_BAD, stride: int = GEN_CTRL_MAX_BAD_LEN + 1) -> int:
    """4-byte words of a control block over `vocab` tokens: header, suppress bitmap, begin-suppress bitmap, n_bad rows of `stride`
    words (the defaults: the largest block there is, the capacity of a controls plan's buffer)"""
    return GEN_CTRL_HEADER_WORDS + 2 * ((int(vocab) + 31) // 32) + int(n_bad) * int(stride)


class GenerationControls:
    """The deterministic logits processors of transformers' generate() that a caller sets per call, as one value object:
    repetition_penalty, no_repeat_ngram_size, min_new_tokens, suppress_tokens, begin_suppress_tokens, bad_words_ids — applied on
    the device by OMNI_OP_GREEDY_CTRL_STEP in transformers' order (include/omni_amd.h).  None everywhere = `neutral`: the call
    runs the plans it always ran.  The constructor checks types and the limits that need no model; `check` the rest (vocabulary,
    max_new_tokens, the special tokens); `pack` writes the control block."""
    __slots__ = ("repetition_penalty", "no_repeat_ngram_size", "min_new_tokens", "suppress_tokens", "begin_suppress_tokens",
                 "bad_words_ids")

    def __init__(self, repetition_penalty=None, no_repeat_ngram_size=None, min_new_tokens=None, suppress_tokens=None,
                 begin_suppress_tokens=None, bad_words_ids=None):
        isint = lambda v: isinstance(v, int) and not isinstance(v, bool)
        p = repetition_penalty
        if p is not None and (isinstance(p, bool) or not isinstance(p, (int, float)) or not p > 0 or math.isinf(p)):
            raise ValueError(f"repetition_penalty must be a float greater than 0, got {p!r}")
        self.repetition_penalty = None if p is None else float(p)
        for name, v in (("no_repeat_ngram_size", no_repeat_ngram_size), ("min_new_tokens", min_new_tokens)):
            if v is not None and (not isint(v) or v < 0):
                raise ValueError(f"{name} must be an integer of at least 0, got {v!r}")
        self.no_repeat_ngram_size, self.min_new_tokens = no_repeat_ngram_size, min_new_tokens

        def tokens(name, v):
            if v is None:
                return ()
            if isinstance(v, torch.Tensor):
                v = v.tolist()
            if isinstance(v, (str, bytes)) or not hasattr(v, "__iter__"):
                raise ValueError(f"{name} must be a list of token ids, got {v!r}")
            v = list(v)
            bad = [t for t in v if not isint(t) or t < 0]
            if bad:
                raise ValueError(f"{name}: token ids must be integers of at least 0, got {bad[0]!r}")
            return tuple(v)
        self.suppress_tokens = tokens("suppress_tokens", suppress_tokens)
        self.begin_suppress_tokens = tokens("begin_suppress_tokens", begin_suppress_tokens)
        if bad_words_ids is not None and (isinstance(bad_words_ids, (str, bytes)) or not hasattr(bad_words_ids, "__iter__")):
            raise ValueError(f"bad_words_ids must be a list of token id lists, got {bad_words_ids!r}")
        words = [tokens("bad_words_ids", w) for w in (bad_words_ids if bad_words_ids is not None else ())]
        if any(len(w) == 0 for w in words):
            raise ValueError("bad_words_ids: an empty sequence bans nothing and is refused")
        long_ = [w for w in words if len(w) > GEN_CTRL_MAX_BAD_LEN]
        if long_:
            raise ValueError(f"bad_words_ids: a sequence of {len(long_[0])} tokens (at most {GEN_CTRL_MAX_BAD_LEN})")
        self.bad_words_ids = tuple(dict.fromkeys(words))          # transformers keys its table by the sequence: duplicates are one entry
        if len(self._multi()) > GEN_CTRL_MAX_BAD:
            raise ValueError(f"bad_words_ids: {len(self._multi())} multi-token sequences (at most {GEN_CTRL_MAX_BAD})")

    @classmethod
    def of(cls, x) -> "GenerationControls":
        """None -> neutral; a GenerationControls -> itself; a dict of GEN_CTRL_KEYS -> its controls (another key: ValueError)"""
        if x is None:
            return cls()
        if isinstance(x, cls):
            return x
        if not isinstance(x, dict):
            raise ValueError(f"generation controls must be a GenerationControls, a dict of {', '.join(GEN_CTRL_KEYS)}, or None; got {x!r}")
        unknown = [k for k in x if k not in GEN_CTRL_KEYS]
        if unknown:
            raise ValueError(f"unknown generation control {unknown[0]!r} (known: {', '.join(GEN_CTRL_KEYS)})")
        return cls(**x)

    def _multi(self):
        return [w for w in self.bad_words_ids if len(w) > 1]

    def _single(self):
        return [w[0] for w in self.bad_words_ids if len(w) == 1]

    @property
    def neutral(self) -> bool:
        """nothing to apply: such a call takes the default plans (same cache key, same ops, same bits)"""
        return (self.repetition_penalty in (None, 1.0) and self.no_repeat_ngram_size is None and self.min_new_tokens in (None, 0)
                and not self.suppress_tokens and not self.begin_suppress_tokens and not self.bad_words_ids)

    def check(self, vocab, max_new_tokens, eos, forced_bos=-1, forced_eos=-1):
        """the checks that need the model: ids inside the vocabulary, min_new_tokens <= max_new_tokens, and no EOS / forced token
        among the suppressed ones (transformers drops [eos] from bad words by itself; a suppressed forced token makes its forced row
        all -inf).  ValueError; returns self."""
        if self.min_new_tokens is not None and self.min_new_tokens > int(max_new_tokens):
            raise ValueError(f"min_new_tokens must be in 0..max_new_tokens ({max_new_tokens}), got {self.min_new_tokens}")
        for name, toks in (("suppress_tokens", self.suppress_tokens), ("begin_suppress_tokens", self.begin_suppress_tokens),
                           ("bad_words_ids", [t for w in self.bad_words_ids for t in w])):
            bad = [t for t in toks if t >= vocab]
            if bad:
                raise ValueError(f"{name}: token id {bad[0]} is outside the vocabulary (0..{vocab - 1})")
        special = {int(eos): "the EOS token"}
        if forced_bos is not None and int(forced_bos) >= 0:
            special.setdefault(int(forced_bos), "the forced BOS token")
        if forced_eos is not None and int(forced_eos) >= 0:
            special.setdefault(int(forced_eos), "the forced EOS token")
        for name, toks in (("suppress_tokens", self.suppress_tokens), ("begin_suppress_tokens", self.begin_suppress_tokens),
                           ("bad_words_ids (as a single-token entry)", self._single())):
            hit = [t for t in toks if t in special]
            if hit:
                raise ValueError(f"{name}: token {hit[0]} is {special[hit[0]]} and cannot be suppressed")
        return self

    def pack(self, vocab, forced_bos=-1) -> torch.Tensor:
        """the control block as i32 words on the host (include/omni_amd.h OMNI_OP_GREEDY_CTRL_STEP): header, suppress bitmap (with
        the single-token bad words), begin-suppress bitmap, bad-word table {length, tokens..} of stride 1 + the longest sequence.
        begin_index as transformers computes it for a decoder that starts from one token: 1, or 2 behind a forced BOS."""
        nw = (int(vocab) + 31) // 32
        multi = self._multi()
        stride = 1 + max(len(w) for w in multi) if multi else 0
        words = torch.zeros(gen_ctrl_words(vocab, len(multi), stride), dtype=torch.int32)
        words[0:1] = torch.tensor([1.0 if self.repetition_penalty is None else self.repetition_penalty], dtype=torch.float32).view(torch.int32)
        words[1] = -1 if self.no_repeat_ngram_size is None else self.no_repeat_ngram_size
        words[2] = self.min_new_tokens or 0
        words[3] = 2 if forced_bos is not None and int(forced_bos) >= 0 else 1
        words[4], words[5] = len(multi), stride

        def bitmap(toks):
            bits = torch.zeros(nw * 32, dtype=torch.int64)
            if toks:
                bits[torch.tensor(sorted(set(toks)))] = 1
            w = (bits.view(nw, 32) << torch.arange(32)).sum(1)                 # < 2^32 in i64
            return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)   # the same 32 bits as i32
        o = GEN_CTRL_HEADER_WORDS
        words[o:o + nw] = bitmap(list(self.suppress_tokens) + self._single())
        words[o + nw:o + 2 * nw] = bitmap(list(self.begin_suppress_tokens))
        for q, w in enumerate(multi):
            r = o + 2 * nw + q * stride
            words[r] = len(w)
            words[r + 1:r + 1 + len(w)] = torch.tensor(w, dtype=torch.int32)
        return words


# ---- closed vocabularies (OMNI_OP_GREEDY_VOCAB_STEP): the ONE Python mirror of the trie block of include/omni_amd.h
VOCAB_HEADER_WORDS = 8             # struct omni_vocab_trie: i32 n_nodes | n_edges | longest | 0 | 0 | 0 | 0 | 0
VOCAB_TRIE_FIELDS = ("n_nodes", "n_edges", "longest", "reserved")
VOCAB_MAX_NODES = 65536            # OMNI_VOCAB_MAX_NODES: nodes of a vocabulary's trie, the root included
VOCAB_MAX_LABEL = 64               # OMNI_VOCAB_MAX_LABEL: tokens of a label


def vocab_trie_words(n_nodes: int = VOCAB_MAX_NODES) -> int:
    """4-byte words of the trie block of a trie of n_nodes nodes (n_nodes - 1 edges): header, first[n_nodes + 1], edge_tok, edge_dst
    (the default: the largest block there is, the capacity of a vocabulary plan's buffer)"""
    return VOCAB_HEADER_WORDS + int(n_nodes) + 1 + 2 * (int(n_nodes) - 1)


def ngram_banned(prefix, n):
    """the tokens transformers' NoRepeatNGramLogitsProcessor(n) bans behind `prefix` (a list of ids)"""
    banned, m = set(), len(prefix)
    if n > 0 and m + 1 >= n:
        tail = prefix[m - (n - 1):]
        for i in range(m - n + 1):
            if prefix[i:i + n - 1] == tail:
                banned.add(prefix[i + n - 1])
    return banned


class CaptionVocabulary:
    """A closed vocabulary of captions as one value object: a set of labels, each a list of token ids in the format
    `Florence2Captioner.score` takes and `FlorenceProcessor.prompt_ids` returns (the generated positions 1..L: the checkpoint's forced
    BOS when it has one, the text, EOS).  Greedy decoding with it (`generate(vocabulary=...)`, OMNI_OP_GREEDY_VOCAB_STEP) returns
    exactly one of the labels per image: transformers' prefix_allowed_tokens_fn for this set, compiled to a trie that the device
    reads at every step.  The constructor deduplicates the labels (`labels`: the distinct ones in their first order, what
    `label_index` counts) and builds the trie; a label that is a prefix of another is fine.  `check` holds the set against a model;
    `pack` writes the trie block."""
    __slots__ = ("labels", "longest", "_children", "_end")

    def __init__(self, labels):
        isint = lambda v: isinstance(v, int) and not isinstance(v, bool)
        if isinstance(labels, torch.Tensor):
            labels = labels.tolist()
        if isinstance(labels, (str, bytes)) or not hasattr(labels, "__iter__"):
            raise ValueError(f"a vocabulary is a list of labels, each a list of token ids; got {labels!r}")
        rows = []
        for lab in labels:
            if isinstance(lab, torch.Tensor):
                lab = lab.tolist()
            if isinstance(lab, (str, bytes)) or not hasattr(lab, "__iter__"):
                raise ValueError(f"vocabulary: a label must be a list of token ids, got {lab!r}")
            lab = tuple(lab)
            if not lab:
                raise ValueError("vocabulary: an empty label")
            if len(lab) > VOCAB_MAX_LABEL:
                raise ValueError(f"vocabulary: a label of {len(lab)} tokens (at most {VOCAB_MAX_LABEL})")
            bad = [t for t in lab if not isint(t) or t < 0]
            if bad:
                raise ValueError(f"vocabulary: token ids must be integers of at least 0, got {bad[0]!r}")
            rows.append(lab)
        if not rows:
            raise ValueError("vocabulary: no label; at least one is needed")
        self.labels = tuple(dict.fromkeys(rows))
        self.longest = max(len(lab) for lab in self.labels)
        self._children, self._end = [{}], {}
        for k, lab in enumerate(self.labels):
            node = 0
            for t in lab:
                nxt = self._children[node].get(t)
                if nxt is None:
                    nxt = len(self._children)
                    self._children[node][t] = nxt
                    self._children.append({})
                node = nxt
            self._end[node] = k
        if len(self._children) > VOCAB_MAX_NODES:
            raise ValueError(f"vocabulary: its trie has {len(self._children)} nodes (at most {VOCAB_MAX_NODES})")

    @classmethod
    def of(cls, x) -> Optional["CaptionVocabulary"]:
        """None -> None (no vocabulary); a CaptionVocabulary -> itself; a list of id lists -> its vocabulary"""
        if x is None or isinstance(x, cls):
            return x
        return cls(x)

    @property
    def n_nodes(self) -> int:
        return len(self._children)

    def children(self, node: int):
        """the allowed next tokens at a node, ascending ([] at a leaf or outside the trie)"""
        return sorted(self._children[node]) if 0 <= node < len(self._children) else []

    def walk(self, tokens, node: int = 0) -> int:
        """the node reached from `node` along `tokens`, -1 once the path leaves the trie"""
        for t in tokens:
            node = self._children[node].get(int(t), -1) if 0 <= node < len(self._children) else -1
            if node < 0:
                return -1
        return node

    def label_of(self, node: int) -> int:
        """index (into `labels`) of the label that ends at `node`, or -1"""
        return self._end.get(int(node), -1)

    def label_index(self, generated, eos) -> int:
        """index of the label a generated row spells (the ids behind the decoder start token, up to and including the first EOS),
        or -1 when it is none of them"""
        row = [int(t) for t in generated]
        if int(eos) not in row:
            return -1
        return self.label_of(self.walk(row[:row.index(int(eos)) + 1]))

    def check(self, vocab, max_new_tokens, eos, forced_bos=-1, forced_eos=-1, ngram=0, start=2):
        """the checks that need the model: ids inside the vocabulary, every label = [forced BOS] text EOS with EOS nowhere else,
        max_new_tokens holds the longest label (else the output would not be a label), a forced EOS token that is not the EOS token
        cannot replace a label's last token (it could only at max_new_tokens == the longest label), and no
        DEAD END: a node where the n-gram ban (size `ngram`) of its own prefix — unique in a trie; the decoder start token `start`
        included — removes every child, so that no label could be completed there.  ValueError; returns self."""
        eos, fb, fe = int(eos), -1 if forced_bos is None else int(forced_bos), -1 if forced_eos is None else int(forced_eos)
        for lab in self.labels:
            bad = [t for t in lab if t >= vocab]
            if bad:
                raise ValueError(f"vocabulary: token id {bad[0]} is outside the vocabulary (0..{vocab - 1})")
            if lab[-1] != eos:
                raise ValueError(f"vocabulary: label {list(lab)} does not end in the EOS token ({eos})")
            if eos in lab[:-1]:
                raise ValueError(f"vocabulary: label {list(lab)} holds the EOS token ({eos}) before its end")
            if fb >= 0 and lab[0] != fb:
                raise ValueError(f"vocabulary: label {list(lab)} does not start with the forced BOS token ({fb}) of this checkpoint")
        if int(max_new_tokens) < self.longest:
            raise ValueError(f"vocabulary: max_new_tokens ({max_new_tokens}) is below the longest label ({self.longest} tokens): the "
                             "output would not be a label")
        # the forced position max_new_tokens is reached by an unfinished row only when it is the last token of a longest label
        if fe >= 0 and fe != eos and int(max_new_tokens) == self.longest:
            raise ValueError(f"vocabulary: the checkpoint forces token {fe} at position max_new_tokens ({max_new_tokens}), which is not "
                             f"its EOS token ({eos}) and would replace the last token of the longest label: give max_new_tokens of at "
                             f"least {self.longest + 1}")
        stack = [(0, [int(start)])]
        while stack:
            node, prefix = stack.pop()
            kids = self._children[node]
            if not kids:
                continue
            forced = (fb >= 0 and len(prefix) == 1) or (fe >= 0 and len(prefix) == int(max_new_tokens))
            if not forced and not set(kids) - ngram_banned(prefix, int(ngram)):
                raise ValueError(f"vocabulary: a dead end behind the prefix {prefix} (decoder start token included): the checkpoint's "
                                 f"no_repeat_ngram_size = {ngram} bans every continuation {sorted(kids)}")
            for t, nxt in kids.items():
                stack.append((nxt, prefix + [t]))
        return self

    def pack(self) -> torch.Tensor:
        """the trie block as i32 words on the host (include/omni_amd.h OMNI_OP_GREEDY_VOCAB_STEP): header {n_nodes, n_edges, longest
        label, 0 x 5}, first[n_nodes + 1], edge_tok (ascending within a node), edge_dst"""
        first, tok, dst = [0], [], []
        for kids in self._children:
            for t in sorted(kids):
                tok.append(t)
                dst.append(kids[t])
            first.append(len(tok))
        n = len(self._children)
        assert len(tok) == n - 1 and VOCAB_HEADER_WORDS + len(first) + 2 * len(tok) == vocab_trie_words(n)
        return torch.tensor([n, len(tok), self.longest, 0, 0, 0, 0, 0] + first + tok + dst, dtype=torch.int32)


FORCE_ROWS = (1, 4, 8)            # candidate rows per crop of a teacher-forced plan (`Florence2Captioner.score`)
LABEL_CAPACITIES = (8, 16, 32)     # label tokens per candidate (T - 1 of such a plan)


def sequence_score(token_logprobs, lengths, labels=None, normalize="mean", forced_bos=None):
    """Score of whole labels from `Florence2Captioner.score`'s output: the sum (normalize="sum") or the mean ("mean") of each
    label's token log-probabilities over its own length.  token_logprobs [..., L], lengths [...] -> f64 tensor [...].
    forced_bos (the checkpoint's `forced_bos_token_id`, `captioner.w.forced_bos`; None or < 0 = none): position 0 is left out when
    it is that token — generation forces it, so its probability says nothing about the text.  labels ([..., L] ids, or nested lists
    indexed the same way): position 0 is compared with forced_bos; without labels every label is taken to start with it (what
    `FlorenceProcessor.prompt_ids` returns does).  A label without a counted position scores 0."""
    if normalize not in ("mean", "sum"):
        raise ValueError(f"normalize must be 'mean' or 'sum', got {normalize!r}")
    lp = torch.as_tensor(token_logprobs).double()
    ln = torch.as_tensor(lengths).long()
    pos = torch.arange(lp.shape[-1])
    counted = pos < ln[..., None]
    if forced_bos is not None and int(forced_bos) >= 0:
        if labels is None:
            skip = torch.ones_like(ln, dtype=torch.bool)
        else:
            def firsts(x, depth):                        # the first token of every label, nested as `lengths` is
                return int(x[0]) if depth == 0 else [firsts(r, depth - 1) for r in x]
            first = labels[..., 0] if isinstance(labels, torch.Tensor) else torch.tensor(firsts(labels, ln.dim()))
            skip = torch.as_tensor(first).reshape(ln.shape) == int(forced_bos)
        counted = counted & ~((pos == 0) & skip[..., None])
    total = torch.where(counted, lp, torch.zeros_like(lp)).sum(-1)
    if normalize == "sum":
        return total
    return total / counted.sum(-1).clamp(min=1)


# ---- visual embeddings and exemplar matching (OMNI_OP_VISUAL_MATCH, csrc/visual_match.hip)
MATCH_MAX_K, MATCH_MAX_D, MATCH_MAX_QUERIES, MATCH_MAX_GALLERY = 8, 4096, 4096, 65536      # the op's limits (include/omni_amd.h)


def embed_op(dtype, x_ptr, ld, y: torch.Tensor, norm: torch.Tensor, n: int, D: int):
    """mode 0: the first D elements of n rows of stride `ld` elements at `x_ptr` (the op's dtype) -> unit vectors y f32 [>= n, D]
    and their norms f32 [>= n]"""
    return L.make_op(L.OP_VISUAL_MATCH, dtype, p=[x_ptr, None, None, None, y.data_ptr(), norm.data_ptr()], i={0: 0, 1: n, 2: ld, 3: D})


def match_ops(q_ptr, g_ptr, part_ptr, idx_ptr, score_ptr, m, n, D, k, split_len=0, part_bytes=0):
    """(mode 1, mode 2) of one match: the same i-slots, so both see the same split"""
    i = {1: m, 2: n, 3: D, 4: k, 5: split_len, 6: part_bytes}
    return (L.make_op(L.OP_VISUAL_MATCH, L.F32, p=[q_ptr, g_ptr, None, None, None, part_ptr], i={0: 1, **i}),
            L.make_op(L.OP_VISUAL_MATCH, L.F32, p=[None, None, None, None, idx_ptr, part_ptr, score_ptr], i={0: 2, **i}))


def match_geometry(m, n, D, k, split_len=0):
    """(query groups, gallery rows per split, splits, bytes of the partials buffer) of a match, asked of the launcher itself
    (omni_visual_match_cfg: the function the launch calls; no device work)"""
    import ctypes
    out = (ctypes.c_longlong * 4)()
    L.check(L.lib().omni_visual_match_cfg(ctypes.byref(match_ops(None, None, None, None, None, m, n, D, k, split_len)[0]), out))
    return tuple(int(v) for v in out)


def check_match_args(queries, gallery, top_k):
    """(m, n, D) of `Florence2Captioner.match`'s arguments, or a ValueError before anything reaches the device"""
    if isinstance(top_k, bool) or not isinstance(top_k, int) or not 1 <= top_k <= MATCH_MAX_K:
        raise ValueError(f"top_k must be an integer in 1..{MATCH_MAX_K}, got {top_k!r}")
    for name, t in (("queries", queries), ("gallery", gallery)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() < 1:
            raise ValueError(f"{name} must be an f32 tensor [.., D], got {type(t).__name__}"
                             + (f" {t.dtype} {tuple(t.shape)}" if isinstance(t, torch.Tensor) else ""))
    D = queries.shape[-1]
    if gallery.shape[-1] != D:
        raise ValueError(f"queries have D = {D}, the gallery has D = {gallery.shape[-1]}")
    m, n = (queries.numel() // D if D else 0), (gallery.numel() // D if D else 0)
    if m < 1 or n < 1:
        raise ValueError(f"an empty side: {m} queries, {n} gallery rows")
    if D % 4 or D > MATCH_MAX_D:
        raise ValueError(f"D = {D}: a multiple of 4 up to {MATCH_MAX_D}")
    if m > MATCH_MAX_QUERIES or n > MATCH_MAX_GALLERY:
        raise ValueError(f"{m} queries x {n} gallery rows: at most {MATCH_MAX_QUERIES} x {MATCH_MAX_GALLERY} per call")
    return m, n, D


@torch.inference_mode()
def match_topk(queries, gallery, top_k=1, device=None):
    """`Florence2Captioner.match` without a captioner (it needs no weights): both launches go to the CURRENT stream of `device`
    (default: the queries' device), where the caller's tensors were produced and the results will be read."""
    m, n, D = check_match_args(queries, gallery, top_k)
    dev = L.require_device(device if device is not None else (queries.device if queries.is_cuda else None), "match")
    with (torch.cuda.device(dev) if dev.type == "cuda" else contextlib.nullcontext()):
        q = queries.reshape(m, D).to(dev).contiguous()
        g = gallery.reshape(n, D).to(dev).contiguous()
        nbytes = match_geometry(m, n, D, top_k)[3]
        part = torch.empty((nbytes // 4,), dtype=torch.int32, device=dev)
        idx = torch.empty((m, top_k), dtype=torch.int32, device=dev)
        score = torch.empty((m, top_k), dtype=torch.float32, device=dev)
        for op in match_ops(q.data_ptr(), g.data_ptr(), part.data_ptr(), idx.data_ptr(), score.data_ptr(), m, n, D, top_k, 0, nbytes):
            L.launch(op)
        return idx.long(), score


# ---- region OCR (OMNI_OP_REGION_OCR, csrc/region_ocr.hip)
OCR_MAX_T, OCR_MAX_R = 2049, 65536                      # the op's limits (include/omni_amd.h)
OCR_INF = 2 ** 31 - 1                                   # a cell without an upper end; the lower one is -2^31


def ocr_slots(T: int) -> int:
    """region slots per row of T tokens: a region is at least one token of content and eight location tokens"""
    return (T - 1) // 9


def tile_cut_op(dtype, img_ptr, origins_ptr, y_ptr, lut_ptr, n, H, W, R, ldo):
    """mode 0: n windows of R x R pixels of the u8 [H, W, 3] frame at the origins i32 [n, 2] -> a caption plan's input rows"""
    return L.make_op(L.OP_REGION_OCR, dtype, p=[img_ptr, origins_ptr, None, None, y_ptr, None, None, lut_ptr],
                     i={0: 0, 1: n, 2: H, 3: W, 4: R, 13: ldo},
                     f={0: CLIP_MEAN[0], 1: CLIP_MEAN[1], 2: CLIP_MEAN[2], 3: CLIP_STD[0], 4: CLIP_STD[1], 5: CLIP_STD[2]})


def region_parse_op(ids_ptr, table_ptr, logp_ptr, cells_ptr, rec_ptr, sum_ptr, rows_ptr, n, T, table_len, R, eos, ld_ids=0, ld_logp=0,
                    slots=None):
    """mode 1: n rows of T ids (and their log-probabilities, or None) -> records i32 [n x M, 16], sums f32 [n x M], counters i32 [n, 4]"""
    return L.make_op(L.OP_REGION_OCR, L.F32, p=[ids_ptr, table_ptr, logp_ptr, None, rec_ptr, sum_ptr, rows_ptr, cells_ptr],
                     i={0: 1, 1: n, 2: T, 3: ocr_slots(T) if slots is None else slots, 4: table_len, 5: ld_ids, 6: ld_logp, 7: R, 8: eos})


def box_slots(T: int) -> int:
    """box slots per row of T tokens (mode 3): a box is four location tokens"""
    return (T - 1) // 4


def box_parse_op(ids_ptr, table_ptr, logp_ptr, cells_ptr, rec_ptr, sum_ptr, rows_ptr, n, T, table_len, R, eos, grammar, ld_ids=0, ld_logp=0,
                 slots=None):
    """mode 3: n rows of T ids (and their log-probabilities, or None) -> box records i32 [n x M, 16], sums f32 [n x M, 2] (phrase,
    box), counters i32 [n, 4]; grammar 0 = phrases with boxes, 1 = boxes only"""
    return L.make_op(L.OP_REGION_OCR, L.F32, p=[ids_ptr, table_ptr, logp_ptr, None, rec_ptr, sum_ptr, rows_ptr, cells_ptr],
                     i={0: L.OCR_MODE_BOXES, 1: n, 2: T, 3: box_slots(T) if slots is None else slots, 4: table_len, 5: ld_ids, 6: ld_logp,
                        7: R, 8: eos, 9: grammar})


def poly_slots(T: int):
    """(polygon slots, vertex slots) per row of T tokens (mode 5): "<loc> <sep> <loc> <sep> ..." fills the first, a vertex is two
    location tokens"""
    return T // 2, (T - 1) // 2


def poly_parse_op(ids_ptr, table_ptr, logp_ptr, cells_ptr, verts_ptr, rec_ptr, sum_ptr, rows_ptr, n, T, table_len, R, eos, ld_ids=0, ld_logp=0,
                  slots=None, vertex_slots=None):
    """mode 5: n rows of T ids (and their log-probabilities, or None) -> vertices i32 [n, V, 2], polygon records i32 [n x P, 16], sums
    f32 [n x P], counters i32 [n, 4]; the class table is FlorenceProcessor.poly_class_table's"""
    P, V = poly_slots(T)
    return L.make_op(L.OP_REGION_OCR, L.F32, p=[ids_ptr, table_ptr, logp_ptr, verts_ptr, rec_ptr, sum_ptr, rows_ptr, cells_ptr],
                     i={0: L.OCR_MODE_POLYS, 1: n, 2: T, 3: P if slots is None else slots, 4: table_len, 5: ld_ids, 6: ld_logp, 7: R, 8: eos,
                        9: V if vertex_slots is None else vertex_slots})


def poly_mask_op(rec_ptr, rows_ptr, verts_ptr, cells_ptr, mask_ptr, count_ptr, n, T, instances, H, W, R):
    """mode 6: mode 5's records, counters and vertices of n rows of T tokens -> tile-local bit masks u32 [n, instances, R, (R + 31) / 32]
    and set bits per pixel row i32 [n, instances, R], clipped to the H x W frame"""
    return L.make_op(L.OP_REGION_OCR, L.F32, p=[rec_ptr, rows_ptr, verts_ptr, None, mask_ptr, count_ptr, None, cells_ptr],
                     i={0: L.OCR_MODE_MASKS, 1: n, 2: T, 3: instances, 4: H, 5: W, 7: R})


def ocr_cells(origins, R: int):
    """The cells table of mode 1 for tiles of R x R pixels at `origins` [(x, y)] (a grid: every x with every y), one row per tile:
    [origin x, origin y, lo x, hi x, lo y, hi y].  Per axis the boundary between neighbouring tiles is the midpoint of their overlap,
    held in DOUBLED pixels (origin + next origin + R) so that it is an integer; lo is inclusive, hi exclusive, and the outermost cells
    have no end (-2^31 / OCR_INF).  A region belongs to the tile whose cell holds the doubled centre of its box on both axes."""
    def axis(vals):
        vs = sorted(set(vals))
        out = {}
        for k, v in enumerate(vs):
            out[v] = (-2 ** 31 if k == 0 else vs[k - 1] + v + R, OCR_INF if k == len(vs) - 1 else v + vs[k + 1] + R)
        return out
    ax, ay = axis([x for x, _ in origins]), axis([y for _, y in origins])
    return [[x, y, *ax[x], *ay[y]] for x, y in origins]


def check_class_table(class_table) -> torch.Tensor:
    """`read_regions`' class table as a contiguous int16-viewed u16 host tensor, or a ValueError"""
    t = class_table
    if isinstance(t, np.ndarray):
        t = torch.from_numpy(t.astype(np.int16) if t.dtype == np.uint16 else t)
    if not isinstance(t, torch.Tensor) or t.dim() != 1 or t.numel() < 1 or t.dtype not in (torch.int16, torch.uint16):
        raise ValueError("class_table must be a non-empty 1-D u16 table (FlorenceProcessor.loc_class_table())")
    return t.view(torch.int16).contiguous()


_DECODE_TUNING = "unset"


def decode_tuning(device=None):
    """The committed tuning table of the decode step's GEMMs (`omniparser_amd/decode_tuning_gfx950.json`, written by
    tools/decode_autotune.py on the MI355X): {shape key: (tile code, split-K count)} for the row counts a merged decode plan can have.
    A decode step is launch-bound (~110 kernels of 5-15 us); the launcher's throughput heuristic cuts its GEMMs into 6 K splits of four
    slices plus a reduce launch where fewer, longer blocks are faster.  Tuning changes the order in which K partials are summed, nothing
    else (the logits' last bits already depend on the row count, see _DecodePlans); OMNI_DECODE_TUNING=0 turns it off; a device that is
    not gfx950, or a missing file, means the heuristic.  NO TABLE IS COMMITTED: measured in round 6 (profiles/r6_s13_decode_autotune.json),
    the best choices beat the heuristic by 2.8 % of a step graph at 128 rows, 0.3-0.5 % at 160-320 rows and nothing at 352 / 384 rows
    (the benched load) — the heuristic stays; the tool and this loader remain for other chips / row counts."""
    global _DECODE_TUNING
    if device is not None and torch.device(device).type == "cuda" and torch.cuda.is_available():
        if not getattr(torch.cuda.get_device_properties(device), "gcnArchName", "").startswith("gfx950"):
            return None
    if _DECODE_TUNING == "unset":
        path = Path(__file__).resolve().parent / "decode_tuning_gfx950.json"
        _DECODE_TUNING = None
        if os.environ.get("OMNI_DECODE_TUNING", "1") != "0" and path.exists():
            _DECODE_TUNING = {k: tuple(v) for k, v in json.loads(path.read_text())["choices"].items()}
    return _DECODE_TUNING


# ------------------------------------------------------------------------------------------ plans
class _Weights:
    """The model's device weights and tables, shared by every plan of a captioner (`cap._wcache`, keyed by (key, dtype[, variant]):
    the tests hand one cache to several captioners).  An entry missing from the cache is built on first use, uploaded through `pb`."""

    def __init__(self, cap: "Florence2Captioner", pb: PlanBuilder):
        self.sd, self.wc, self.dt, self.pb = cap.w.sd, cap._wcache, cap.dtype, pb

    def cached(self, ck, build):
        if ck not in self.wc:
            self.wc[ck] = build()
        return self.wc[ck]

    def packed(self, key, make, dma=False):
        """(packed weight, f32 bias or None) of make() = (weight, bias or None): format B of the LDS-DMA GEMM (dma) or conv layout"""
        def build():
            wt, b = make()
            return (self.pb.pack_weight_dma(wt) if dma else self.pb.pack_weight(wt if wt.dim() == 4 else wt[:, :, None, None]),
                    self.pb.upload(b.float()) if b is not None else None)
        return self.cached((key, self.dt, "dma") if dma else (key, self.dt), build)

    def linear(self, keys, bias=True, dma=False):
        """`packed` of the nn.Linear layers `keys` concatenated along the output axis (q|k|v, k|v: one GEMM)"""
        sd = self.sd
        return self.packed("|".join(keys), lambda: (torch.cat([sd[k + ".weight"] for k in keys], 0),
                                                    torch.cat([sd[k + ".bias"] for k in keys], 0) if bias else None), dma)

    def f32(self, key):
        return self.cached((key, "f32"), lambda: self.pb.upload(self.sd[key].float()))

    def token_tables(self):
        """(token embedding table, decoder position table) in the plan dtype: the decoder step and the prompt gather read the first"""
        lm, tdt = "model.language_model.", torch_dtype(self.dt)
        return self.cached(("dectab", self.dt), lambda: (self.pb.upload(self.sd[lm + "shared.weight"].to(tdt)),
                                                         self.pb.upload(self.sd[lm + "decoder.embed_positions.weight"].to(tdt))))

    def dwconv(self, key):
        """depthwise 3x3 convolution: weight [C,1,3,3] -> [3][3][C] in the plan dtype, f32 bias"""
        wt, b = self.sd[key + ".weight"], self.sd[key + ".bias"]
        return self.cached((key, self.dt), lambda: (self.pb.upload(wt[:, 0].permute(1, 2, 0).contiguous().to(torch_dtype(self.dt))),
                                                    self.pb.upload(b.float())))

    def layernorm(self, key, x, out, rows, C, add=None, y2=None, period=0, omode=0, eps=1e-5):
        """OMNI_OP_LAYERNORM over `rows` rows of C channels (device addresses x, add, out, y2) with the affine parameters of `key`"""
        return L.make_op(L.OP_LAYERNORM, self.dt, p=[x, add, self.f32(key + ".weight").data_ptr(), self.f32(key + ".bias").data_ptr(), out, y2],
                         i={0: rows, 1: 1, 3: C, 5: period, 6: omode}, f={0: eps})


class _StepPlans:
    """The decoder-step plan over B rows (embedding, 6 BART decoder layers with self-KV cache and fixed cross-KV, lm_head, logits
    processors + arg-max on the device) and its state: shared by _CaptionPlans (encode + decode of one micro-batch) and _DecodePlans.

    beam = (k, length_penalty, early_stopping): beam search over B crops = B k decoder rows (crop b owns rows [b k, b k + k)); the
    cross-attention reads the crop's single cross-K / V row (OMNI_OP_ATTN_DECODE i12 = k), the self-attention reads its history
    through a position table that OMNI_OP_BEAM_STEP rewrites when beams are reordered (no K / V is copied), and OMNI_OP_BEAM_STEP
    replaces OMNI_OP_GREEDY_STEP.  `finished` then holds the per-crop frozen flags (nothing can change any more).  beam = None
    builds the greedy plan, op for op as before.

    scores (greedy only): the plan also owns `logp` f32 [B, T], OMNI_OP_GREEDY_STEP p4 — the log-probability of every emitted token
    (include/omni_amd.h).  Off, the greedy op keeps p4 = NULL and there is no such buffer.

    force = M (no beam, no scores): a teacher-forced plan over B crops x M candidate rows (crop b owns rows [b M, b M + M)) that
    SCORES given texts instead of generating one.  The cross-attention shares the crop's cross-K / V row (i12 = M) as a beam plan
    with k = M does, the self-attention has no position table (every row keeps its own cache row), and OMNI_OP_GREEDY_STEP takes
    its target-score form (p5): `ids` [B M, T] is an INPUT (column 0 the decoder start token, columns 1..len the candidate's
    labels, `set_targets`), `tlen` i32 [B M] the label lengths (0 = unused row), `logp` f32 / `top1` i32 [B M, T] the outputs.
    There is no `finished`; max_new is the label capacity T - 1."""
    beam = None
    logp = None
    force = None
    ctrl = None
    node = None
    trie = None

    def _build_step(self, cap, B, max_new, S, cross_kv, ws=None, beam=None, nkeys=None, scores=False, force=None, controls=False,
                    vocab=False):
        """nkeys: i32 [crops] valid encoder keys per crop (a prompt shorter than the plan's text capacity: OMNI_OP_ATTN_DECODE p7 of
        the cross-attention), or None = all S
        controls (greedy only): the plan owns `ctrl`, an i32 buffer of the largest control block (`gen_ctrl_words`), and ends in
        OMNI_OP_GREEDY_CTRL_STEP instead of OMNI_OP_GREEDY_STEP; `set_controls` uploads a call's block before its first step
        vocab (greedy only, with or without scores): the plan owns `node` i32 [B] (every row's trie node, zeroed by `reset`) and `trie`,
        an i32 buffer of the largest trie block (`vocab_trie_words`), and ends in OMNI_OP_GREEDY_VOCAB_STEP; `set_vocabulary` uploads a
        call's block before its first step"""
        w, dev, dt = cap.w, cap.device, cap.dtype
        sd = w.sd
        D, nh, lm = w.d_model, w.n_heads, "model.language_model."
        self.T = max_new + 1
        self.beam = beam
        assert not (force and (beam or scores)), "a teacher-forced plan neither searches nor generates"
        assert not (controls and (beam or force)), "generation controls are a greedy-decoding feature"
        assert not (vocab and (beam or force or controls)), "a closed vocabulary is a greedy-decoding feature without generation controls"
        self.force = force
        kb = beam[0] if beam else (force or 1)
        crops, B = B, B * kb                               # B = decoder rows from here on
        W = _Weights(cap, PlanBuilder(dev, dt))            # weights / tables missing from the model's cache are uploaded through its builder
        pd_ = PlanBuilder(dev, dt)
        pd_.ws = ws
        if isinstance(self, _DecodePlans):
            pd_.conv_tuning = decode_tuning(dev)          # merged decode plans only: the per-micro-batch step plans keep the heuristic
        self.pd = pd_
        T = self.T
        self.B = crops
        self.ids = pd_.raw((B, T), torch.int32)
        if beam:
            self.table = pd_.raw((B, T), torch.int32)
            self.run_score = pd_.raw((B,), torch.float32)
            self.fin_ids = pd_.raw((crops, kb, T), torch.int32)
            self.state = pd_.raw((crops * (3 * kb + 2),), torch.int32)     # layout: include/omni_amd.h OMNI_OP_BEAM_STEP p7
            self.fin_score = self.state[:crops * kb].view(torch.float32).view(crops, kb)
            self.fin_len = self.state[2 * crops * kb:3 * crops * kb].view(crops, kb)
            self.heuristic = self.state[3 * crops * kb:3 * crops * kb + crops]
            self.finished = self.state[3 * crops * kb + crops:]
        elif force:
            self.finished = None
            self.tlen = pd_.raw((B,), torch.int32)
            self.top1 = pd_.raw((B, T), torch.int32)
        else:
            self.finished = pd_.raw((B,), torch.int32)
        assert not (scores and beam), "token scores are a greedy-decoding output (beam search returns sequences_scores)"
        self.logp = pd_.raw((B, T), torch.float32) if scores or force else None
        self.step = pd_.raw((1,), torch.int32)
        if controls:
            self.ctrl = pd_.raw((gen_ctrl_words(w.vocab),), torch.int32)
            self.ctrl.zero_()
            neutral = GenerationControls().pack(w.vocab, w.forced_bos)
            self.ctrl[:neutral.numel()].copy_(neutral)
            if dev.type == "cuda":
                torch.cuda.current_stream(dev).synchronize()       # omni_plan_create reads the block's header back
        if vocab:
            self.node = pd_.raw((B,), torch.int32)
            self.node.zero_()
            self.trie = pd_.raw((vocab_trie_words(),), torch.int32)
            self.trie.zero_()
            one = CaptionVocabulary([([w.forced_bos] if w.forced_bos >= 0 else []) + [w.eos]]).pack()
            self.trie[:one.numel()].copy_(one)
            if dev.type == "cuda":
                torch.cuda.current_stream(dev).synchronize()       # omni_plan_create reads the block's header back
        esz = 4 if dt == L.F32 else 2

        def dlinear(key, xin: View, out: View, act=L.ACT_NONE, res=None, keys=None):
            return pd_.conv(xin, *W.linear(keys or [key]), out, 1, act=act, res=res)

        def dln(key, xin: View, out: View):
            pd_.add_op(W.layernorm(key, xin.ptr, out.ptr, B, D))

        table, dpos = W.token_tables()
        pd_.keep += [table, dpos]
        e = pd_.alloc(B, 1, 1, D)
        pd_.add_op(L.make_op(L.OP_EMBED_STEP, dt, p=[table.data_ptr(), dpos.data_ptr(), self.ids.data_ptr(), None, e.ptr,
                                                     None, self.step.data_ptr()],
                             i={0: B, 3: D, 4: T, 5: 2}, f={0: w.embed_scale}))
        xd = pd_.alloc(B, 1, 1, D)
        dln(lm + "decoder.layernorm_embedding", e, xd)
        dqkv = pd_.alloc(B, 1, 1, 3 * D)
        dq = pd_.alloc(B, 1, 1, D)
        da = pd_.alloc(B, 1, 1, D)
        dt_ = pd_.alloc(B, 1, 1, D)
        dffn = pd_.alloc(B, 1, 1, sd[lm + "decoder.layers.0.fc1.weight"].shape[0])
        self.self_k = [pd_.alloc(B, T, 1, D) for _ in range(w.dec_layers)]
        self.self_v = [pd_.alloc(B, T, 1, D) for _ in range(w.dec_layers)]
        for l in range(w.dec_layers):
            pre = f"{lm}decoder.layers.{l}."
            dlinear(None, xd, dqkv, keys=[pre + "self_attn.q_proj", pre + "self_attn.k_proj", pre + "self_attn.v_proj"])
            pd_.add_op(L.make_op(L.OP_ATTN_DECODE, dt,
                                 p=[dqkv.ptr, dqkv.ptr, dqkv.ptr, self.self_k[l].ptr, da.ptr, self.self_v[l].ptr, self.step.data_ptr()]
                                 + ([self.table.data_ptr()] if beam else []),
                                 i={0: 3 * D, 1: 0, 2: 3 * D, 3: D, 4: 2 * D, 5: D, 6: nh, 7: 0, 8: T, 9: D, 10: B, 11: D},
                                 f={0: 64 ** -0.5}))
            dlinear(pre + "self_attn.out_proj", da, dt_, res=xd)
            dln(pre + "self_attn_layer_norm", dt_, xd)
            dlinear(pre + "encoder_attn.q_proj", xd, dq)
            kv = self.cross_kv[l]
            pd_.add_op(L.make_op(L.OP_ATTN_DECODE, dt,
                                 p=[dq.ptr, None, None, kv.ptr, da.ptr, kv.ptr + D * esz, None]
                                 + ([nkeys.data_ptr()] if nkeys is not None else []),
                                 i={0: D, 1: 0, 2: 0, 3: 0, 4: 0, 5: D, 6: nh, 7: S, 8: S, 9: D, 10: B, 11: 2 * D,
                                    **({12: kb} if beam or kb > 1 else {})},
                                 f={0: 64 ** -0.5}))
            dlinear(pre + "encoder_attn.out_proj", da, dt_, res=xd)
            dln(pre + "encoder_attn_layer_norm", dt_, xd)
            dlinear(pre + "fc1", xd, dffn, act=L.ACT_GELU)
            dlinear(pre + "fc2", dffn, dt_, res=xd)
            dln(pre + "final_layer_norm", dt_, xd)
        logits = pd_.alloc(B, 1, 1, w.vocab)
        self.logits = logits
        wp, _ = W.packed("lm_head", lambda: (sd["lm_head.weight"], None))
        pd_.conv(xd, wp, None, logits, 1)
        flb = None
        if "final_logits_bias" in sd:
            flb = W.f32("final_logits_bias")
            pd_.keep.append(flb)
        if beam:
            pd_.add_op(L.make_op(L.OP_BEAM_STEP, dt,
                                 p=[logits.ptr, flb.data_ptr() if flb is not None else None, self.ids.data_ptr(), self.run_score.data_ptr(),
                                    self.table.data_ptr(), self.fin_ids.data_ptr(), self.step.data_ptr(), self.state.data_ptr()],
                                 i={0: crops, 1: w.vocab, 2: w.vocab, 3: T, 4: max_new, 5: w.ngram, 6: kb, 7: w.eos, 8: w.pad,
                                    9: w.forced_bos, 10: w.forced_eos, 11: 1, 12: _EARLY_STOPPING_CODE[beam[2]]},
                                 f={0: beam[1]}))
        elif force:                                        # the target-score form: the processors' slots stay empty, p3 is not used
            pd_.add_op(L.make_op(L.OP_GREEDY_STEP, dt,
                                 p=[logits.ptr, flb.data_ptr() if flb is not None else None, self.ids.data_ptr(), None,
                                    self.logp.data_ptr(), self.tlen.data_ptr(), self.step.data_ptr(), self.top1.data_ptr()],
                                 i={0: B, 1: w.vocab, 2: w.vocab, 3: T, 4: max_new, 6: w.bos, 7: w.eos, 8: w.pad, 9: -1, 10: -1, 11: 1}))
        elif controls:                                     # the same slots + the control block, read on the device at every step
            pd_.add_op(L.make_op(L.OP_GREEDY_CTRL_STEP, dt,
                                 p=[logits.ptr, flb.data_ptr() if flb is not None else None, self.ids.data_ptr(),
                                    self.finished.data_ptr(), self.logp.data_ptr() if scores else None, None, self.step.data_ptr(),
                                    self.ctrl.data_ptr()],
                                 i={0: B, 1: w.vocab, 2: w.vocab, 3: T, 4: max_new, 5: w.ngram, 6: w.bos, 7: w.eos, 8: w.pad,
                                    9: w.forced_bos, 10: w.forced_eos, 11: 1, 12: self.ctrl.numel() * 4}))
        elif vocab:                                        # the same slots + the rows' trie nodes and the trie block
            pd_.add_op(L.make_op(L.OP_GREEDY_VOCAB_STEP, dt,
                                 p=[logits.ptr, flb.data_ptr() if flb is not None else None, self.ids.data_ptr(),
                                    self.finished.data_ptr(), self.logp.data_ptr() if scores else None, self.node.data_ptr(),
                                    self.step.data_ptr(), self.trie.data_ptr()],
                                 i={0: B, 1: w.vocab, 2: w.vocab, 3: T, 4: max_new, 5: w.ngram, 6: w.bos, 7: w.eos, 8: w.pad,
                                    9: w.forced_bos, 10: w.forced_eos, 11: 1, 12: self.trie.numel() * 4}))
        else:
            pd_.add_op(L.make_op(L.OP_GREEDY_STEP, dt,
                                 p=[logits.ptr, flb.data_ptr() if flb is not None else None, self.ids.data_ptr(),
                                    self.finished.data_ptr(), self.logp.data_ptr() if scores else None, None, self.step.data_ptr()],
                                 i={0: B, 1: w.vocab, 2: w.vocab, 3: T, 4: max_new, 5: w.ngram, 6: w.bos, 7: w.eos, 8: w.pad,
                                    9: w.forced_bos, 10: w.forced_eos, 11: 1}))
        self.step_flops = pd_.flops
        self.step_plan = pd_.build()
        self.start_token = w.start
        self.pad_token = w.pad

    def reset(self):
        if self.beam:
            self._reset_beams()
            return
        if self.force:                                     # every row unused (tlen 0) until `set_targets`
            self.ids.fill_(self.pad_token)
            self.ids[:, 0] = self.start_token
            self.tlen.zero_()
            self.logp.zero_()
            self.top1.zero_()
            self.step.zero_()
            return
        self.ids.zero_()
        self.ids[:, 0] = self.start_token
        self.finished.zero_()
        if self.logp is not None:
            self.logp.zero_()
        if self.node is not None:                          # every row at the root
            self.node.zero_()
        self.step.zero_()

    def _reset_beams(self):
        """hf _beam_search's initial state: running scores [0, -1e9, ...], finished scores -1e9, sequences = start token + pad, the
        early-stop heuristic unsatisfied; every position of a row in its own cache row."""
        k, B = self.beam[0], self.B
        self.ids.fill_(self.pad_token)
        self.ids[:, 0] = self.start_token
        self.table.copy_(torch.arange(B * k, dtype=torch.int32, device=self.table.device)[:, None].expand(B * k, self.T))
        self.run_score.view(B, k)[:, 0] = 0.0
        self.run_score.view(B, k)[:, 1:] = -1.0e9
        self.fin_ids.fill_(self.pad_token)
        self.fin_ids[:, :, 0] = self.start_token
        self.state.zero_()
        self.fin_score.fill_(-1.0e9)
        self.heuristic.fill_(1)
        self.step.zero_()

    def set_targets(self, ids: torch.Tensor, tlen: torch.Tensor):
        """a force plan's inputs on the current stream: ids i32 [B M, T] (start token, labels, pad) and tlen i32 [B M], from the host"""
        assert self.force and tuple(ids.shape) == tuple(self.ids.shape) and tuple(tlen.shape) == tuple(self.tlen.shape)
        self.ids.copy_(ids, non_blocking=True)
        self.tlen.copy_(tlen, non_blocking=True)

    def set_controls(self, block: torch.Tensor):
        """a controls plan's block on the current stream: `GenerationControls.pack` words from the host.  Words of the buffer
        behind the block keep what they held; no header makes the kernel read them."""
        assert self.ctrl is not None and block.dtype == torch.int32 and block.numel() <= self.ctrl.numel()
        self.ctrl[:block.numel()].copy_(block, non_blocking=True)

    def set_vocabulary(self, block: torch.Tensor):
        """a vocabulary plan's trie block on the current stream: `CaptionVocabulary.pack` words from the host.  Words of the buffer
        behind the block keep what they held; no header makes the kernel read them."""
        assert self.trie is not None and block.dtype == torch.int32 and block.numel() <= self.trie.numel()
        self.trie[:block.numel()].copy_(block, non_blocking=True)

    def result_ids(self, n: int) -> torch.Tensor:
        """device ids of the first n crops: the greedy rows, or the best finished hypothesis of each crop"""
        return self.fin_ids[:n, 0] if self.beam else self.ids[:n]

    def result_logp(self, n: int) -> torch.Tensor:
        """device token log-probabilities of the first n crops, aligned with `result_ids` (a plan built with scores=True)"""
        return self.logp[:n]

    def snapshot(self, n: int):
        """stream-ordered copy of the first n result rows for a later read-back: the ids, or (ids, logp) from a scores plan"""
        ids = self.result_ids(n).clone()
        return ids if self.logp is None else (ids, self.result_logp(n).clone())

    def _warm_up_and_capture(self, cap, *plans):
        """run the plans once on the captioner's stream (first launches outside a capture), then capture each as a hipGraph"""
        if cap.device.type == "cuda":
            torch.cuda.synchronize(cap.device)      # allocations / uploads ran on the current stream: order them before cap.stream
        if cap.use_graph:
            self.reset()
            for p in plans:
                p.run(cap.stream)
            cap.stream.synchronize()
            for p in plans:
                p.capture(cap.stream)
            cap.stream.synchronize()


class _DecodePlans(_StepPlans):
    """Decode for the crops of SEVERAL caption micro-batches at once.  The encode side of a batch of screenshots runs in micro-batches
    of <= 128 crops (~25 GB of activations each at 768x768 with activation reuse, 60 GB without); the decode side is 20 steps of ~110 small kernels whose cost hardly
    depends on the row count (launch-bound GEMMs over 128 rows) — per micro-batch that was 29 ms, 80 ms of a 750 ms step.  Here the
    cross-attention K / V of every micro-batch are copied (6 x 460 MB per 128 crops, ~1 ms) into the row range of ONE decode plan over
    B rows, which then runs its 20 steps once.  Rows are independent: ids per crop are what the per-micro-batch decode produces
    (same kernels; the split-K choice of the step GEMMs, hence the last bits of the logits, depends on the row count).

    n_txt: text capacity of the micro-batches' plans when the prompt is an input (`_CaptionPlans`); `nkeys` is then the merged
    table of valid encoder keys per crop, copied from the micro-batches like the K / V (`_encode_into`)."""

    def __init__(self, cap: "Florence2Captioner", B: int, R: int, max_new: int, beam=None, n_txt=None, scores=False, vocab=False):
        w, dev, dt = cap.w, cap.device, cap.dtype
        self.B, self.R = B, R
        S = (R // 32) ** 2 + 1 + (len(PROMPT_IDS) if n_txt is None else n_txt)
        self.S = S
        self.n_txt = n_txt
        pk = PlanBuilder(dev, dt)
        self.nkeys = None
        if n_txt is not None:
            self.nkeys = pk.raw((B,), torch.int32)
            self.nkeys.fill_(S)        # rows behind the last crop are decoded too: all (zero) keys, as without a table
        # zero-initialised: the rows behind the last crop are never written (the micro-batches copy their own rows only) but ARE decoded;
        # recycled allocator memory there can hold NaN bit patterns, whose logits are all-NaN rows (found by the one-process GPU suite)
        self.cross_kv = [pk.alloc(B, S, 1, 2 * w.d_model, zero=True) for _ in range(w.dec_layers)]
        self._keep = pk.keep
        self._build_step(cap, B, max_new, S, self.cross_kv, beam=beam, nkeys=self.nkeys, scores=scores, vocab=vocab)
        self.free_evt = None       # recorded behind the decode that last used this plan on another stream (pipelined batches)
        self._warm_up_and_capture(cap, self.step_plan)


class _CaptionPlans(_StepPlans):
    """Static plans for B crops at resolution R.

    arena: another _CaptionPlans of the same resolution and a capacity >= B whose BUFFERS this one uses (round 6).  Such a plan set is
    encode-only: the same op list over the first B rows of every tensor of `arena` (PlanBuilder._from_arena), captured as its own
    hipGraph — the last micro-batch of a caption batch then computes exactly its own rows instead of a padded bucket (89 rows instead
    of 96 at the benched load), without a second set of activations (~19 GB at 96 rows).  Built on demand by `encode_rows`.

    n_txt = None: the default prompt, a constant block of len(PROMPT_IDS) embedding rows baked into the plan (no table, no mask:
    op for op what it always was).  n_txt in TEXT_CAPACITIES: the prompt is a plan INPUT like the pixels — `prompt_ids`
    i32 [B, n_txt] (right-padded with the pad token) and `nkeys` i32 [B] = n_img + prompt length, written by `set_prompt` on the
    plan's stream before a replay.  OMNI_OP_ASSEMBLE gathers the embedding rows on the device, the encoder self-attention and the
    decoder cross-attention give keys at or beyond nkeys[b] no weight.  Padded positions are computed as queries (they hold the
    pad token's embedding, attend to the valid keys, stay finite) and are read by nobody."""

    def __init__(self, cap: "Florence2Captioner", B: int, R: int, max_new: int, arena: Optional["_CaptionPlans"] = None, stream=None,
                 beam=None, n_txt=None, scores=False, force=None, controls=False, vocab=False, embed=False):
        w, dev, dt = cap.w, cap.device, cap.dtype
        if arena is not None:
            n_txt = arena.n_txt
        self.embed = bool(embed)
        self.n_txt = n_txt
        sd = w.sd
        self.B, self.R, self.T = B, R, max_new + 1
        pb = PlanBuilder(dev, dt)
        pb.reuse = bool(cap.reuse_activations)
        if arena is not None:
            assert arena.R == R and arena.B >= B and arena.arena is None
            pb.arena = iter(arena.pb.alloc_log)
        self.arena = arena
        self._row_plans = {}      # n -> encode-only plan set of exactly n rows in THIS plan set's buffers (encode_rows), LRU
        self.pb = pb
        V = pb.V
        W = _Weights(cap, pb)

        # f32 plans run the encode-side linear layers on the pre-split LDS-DMA GEMM (csrc/gemm_dma.hip): weights in format B,
        # inputs written pre-split by their producers.  OMNI_GEMM_DMA=0 keeps every layer on the register-staged kernels.
        use_dma = dt == L.F32 and pb.split and os.environ.get("OMNI_GEMM_DMA", "1") != "0"
        self.use_dma = use_dma
        # format B is decided per producer / consumer GROUP, not per layer: a DaViT stage (or the encoder) uses it only when EVERY
        # linear layer fed by its LayerNorm / GELU / attention outputs takes the LDS-DMA GEMM (N % 128 == 0, K % 32 == 0), i.e. when
        # the width is a multiple of 128 — true for all Florence-2 widths (128..1024, 768); narrower stand-ins stay on f32 tensors
        grp = {"dma": use_dma}

        def tokens(v: View) -> View:
            return View(v.t.view(v.B, v.H * v.W, 1, v.ld), v.coff, v.C, v.fmt)

        def linear(key, x: View, out: View, act=L.ACT_NONE, res=None, bias=True, keys=None, out_split=False):
            """nn.Linear.  With the LDS-DMA GEMM an f32 input is converted to format B IN PLACE first (callers only pass
            tensors whose f32 content nobody else reads); out_split: the epilogue writes format B for the next GEMM."""
            keys = keys or [key]
            n_out, k_in = out.C, x.C
            dma = grp["dma"] and n_out % 128 == 0 and k_in % 32 == 0 and x.ld % 16 == 0 and x.coff % 16 == 0
            assert dma or x.fmt != "split", f"{keys}: split input for a layer that cannot take the LDS-DMA GEMM"
            wp, bp = W.linear(keys, bias, dma)
            if dma and x.fmt != "split":
                pb.split_convert(x)
            xt, ot = tokens(x), tokens(out)
            pb.conv(xt, wp, bp, ot, 1, act=act, res=tokens(res) if res is not None else None, out_split=dma and out_split)
            out.fmt = ot.fmt
            return out

        def layernorm(key, x: View, out: View, add=None, period=0, eps=1e-5, split=None):
            """split=None: f32 output; split=out: write format B instead (the only consumer is an LDS-DMA GEMM);
            split=<other View>: f32 into `out` AND format B into that view (post-LN rows that are also a residual)."""
            rows = x.B * x.H * x.W
            omode, y2 = 0, None
            if grp["dma"] and split is not None and x.C % 16 == 0:
                omode, y2 = (1, None) if split is out else (2, split)
            pb.add_op(W.layernorm(key, x.ptr, out.ptr, rows, x.C, add=add.data_ptr() if add is not None else None,
                                  y2=y2.ptr if y2 is not None else None, period=period, omode=omode, eps=eps))
            out.fmt = "split" if omode == 1 else "f32"
            if y2 is not None:
                y2.fmt = "split"
            return out

        def dwconv(key, x: View, out: View):
            wp, bp = W.dwconv(key)
            pb.keep += [wp, bp]
            pb.add_op(L.make_op(L.OP_DWCONV3, dt, p=[x.ptr, wp.data_ptr(), bp.data_ptr(), None, out.ptr],
                                i={0: x.B, 1: x.H, 2: x.W, 3: x.C}))
            return out

        # x + dwconv(x) and the LayerNorm behind it as ONE strip kernel (csrc/caption_ops.hip::dwln_strip_kernel) wherever it exists
        # (f32 plans, C = 128 / 256 / 512: DaViT stages 0-2); Florence2Captioner.fuse_dwln = False keeps the two separate kernels
        fuse_env = cap.fuse_dwln
        # the attention kernels write their output pre-split for the projection GEMM (no split_convert pass: 22.5 -> 0.3 ms per step on
        # the MI355X, BENCH_r02 extra.ab_opt_in_kernels); Florence2Captioner.attn_split_out = False = f32 output + in-place conversion
        attn_split = use_dma and cap.attn_split_out

        def dwconv_ln(conv_key, norm_key, x: View, y1: View, hout: View):
            """x1 = x + dwconv(x); h = LN(x1) — one kernel (the conv result never leaves registers before the statistics)."""
            if not (fuse_env and dt == L.F32 and x.C in (128, 256, 512)):
                dwconv(conv_key, x, y1)
                return layernorm(norm_key, y1, hout, split=hout)      # hbuf only feeds qkv / fc1
            wp, bp = W.dwconv(conv_key)
            pb.keep += [wp, bp]
            pb.add_op(L.make_op(L.OP_DWCONV3_LN, dt,
                                p=[x.ptr, wp.data_ptr(), bp.data_ptr(), hout.ptr, y1.ptr,
                                   W.f32(norm_key + ".weight").data_ptr(), W.f32(norm_key + ".bias").data_ptr()],
                                i={0: x.B, 1: x.H, 2: x.W, 3: x.C, 6: 1 if grp["dma"] else 0}, f={0: 1e-5}))
            hout.fmt = "split" if grp["dma"] else "f32"
            return hout

        # ---------------- input + vision tower
        self.x_in = pb.alloc(B, R, R, V, zero=True)
        x = self.x_in
        vt = "model.vision_tower."
        self.chan_ws = None
        self.fold_stages = []        # DaViT stages whose channel blocks run folded (Florence2Captioner.fold_chan_proj)
        self.stage_out = []          # output of every DaViT stage (valid after the encode plan unless cap.reuse_activations: each stage owns its buffers)
        for s in range(4):
            C = w.embed_dim[s]
            grp["dma"] = use_dma and C % 128 == 0
            k, st, pd = w.patch[s]
            Ho = (x.H + 2 * pd - k) // st + 1
            conv_key = f"{vt}convs.{s}.conv"
            if w.prenorm[s]:
                xn = pb.alloc(B, x.H, x.W, x.C)
                layernorm(f"{vt}convs.{s}.norm", x, xn)
                cur = pb.alloc(B, Ho, Ho, C)
                wp, bp = W.packed(conv_key, lambda: (sd[conv_key + ".weight"], sd[conv_key + ".bias"]))
                pb.conv(xn, wp, bp, cur, k, st, pd)
                pb.release(xn, *([] if x is self.x_in else [x]))   # reuse_activations: the previous stage's output has had its last reader
            else:
                t0 = pb.alloc(B, Ho, Ho, C)
                if cap.patch_rows and dt == L.F32 and pb.split and V == 4 and k <= 8 and x is self.x_in:
                    # the 7 x 7 / stride-4 patch embedding over the 3 (stored: 4) input channels as a 7 x 1 convolution over 8 consecutive
                    # pixels on the split-f16 MFMA kernel (PlanBuilder.conv_patch) instead of K = 196 on the exact-f32 one (81 TF/s)
                    wp, bp = W.cached((conv_key, dt, "patch"), lambda: (pb.pack_weight_patch(sd[conv_key + ".weight"], V),
                                                                         pb.upload(sd[conv_key + ".bias"].float())))
                    pb.conv_patch(x, wp, bp, t0, k, st, pd)
                else:
                    wp, bp = W.cached((conv_key, dt, "pad"), lambda: (pb.pack_weight(sd[conv_key + ".weight"], cin_pad=V),
                                                                       pb.upload(sd[conv_key + ".bias"].float())))
                    pb.conv(x, wp, bp, t0, k, st, pd)
                cur = pb.alloc(B, Ho, Ho, C)
                layernorm(f"{vt}convs.{s}.norm", t0, cur)
                pb.release(t0)               # (x is the plan's input here: the crop kernels write it, never released)
            H = Ho
            N = H * H
            A_, B_ = cur, pb.alloc(B, H, H, C)
            hbuf = pb.alloc(B, H, H, C)
            qkv = pb.alloc(B, H, H, 3 * C)
            att = pb.alloc(B, H, H, C)
            # the FFN of the C = 128 stage is one kernel whose hidden activations stay in registers (csrc/gemm_dma.hip::mlp_fused_kernel):
            # no [B, H, H, 4C] tensor (9.7 GB of a 128-crop plan at 768x768), 12 instead of 44 bytes of HBM traffic per token-channel
            mlp_one = grp["dma"] and cap.fuse_mlp and C == 128 and sd[f"{vt}blocks.{s}.0.spatial_block.ffn.fc1.weight"].shape[0] == 512
            ffn = None if mlp_one else pb.alloc(B, H, H, 4 * C)
            # fold rule: the fold's bytes and MACs grow with C^2 per image, what it saves with N * C — worth it from N >= 4 C on;
            # whole 256-row GEMM tiles per image.  768x768 crops: stages 0-2; 64x64 crops: none
            fold = bool(cap.fold_chan_proj) and grp["dma"] and dt == L.F32 and C % 128 == 0 and N % 256 == 0 and N >= 4 * C
            # folded stages keep their scores as 256-token partials — the row tile of the q|k GEMM, whose scores epilogue writes one partial
            # per tile and group (cap.chan_scores_in_gemm) — on BOTH sides of that switch: the standalone scores kernel then gives the same
            # bits.  The chunk (i5) stays 1024 in every stage; folded stages carry the partial size in OMNI_OP_CHAN_ATTN i10
            chunk_tokens = 1024
            partial_tokens = 256 if fold else 0
            chunks = (N + (partial_tokens or chunk_tokens) - 1) // (partial_tokens or chunk_tokens)
            cws = pb.raw((B * w.groups[s] * chunks * 1024,), torch.float32, zero=False)
            scores_in_gemm = fold and bool(cap.chan_scores_in_gemm)
            # Wv folded in as well (cap.fold_chan_v): y = h . (W'_b Wv)^T + b''_b — the v launch and the v tensor go, the fold pays
            # C^3 MACs per image and block where the v launch pays N C^2.  Rule: every folded stage (N >= 4 C; measured per stage)
            fold_v = fold and bool(cap.fold_chan_v) and N >= 4 * C
            fold_wf = fold_wb = fold_sc = fold_mx = fold_bias = None
            if fold:                                      # stage scratch, image-major: an exact-row twin uses the first n images' part
                # fold_v: the per-image bias table b''_b [B][C] lies behind the B matrices (OMNI_OP_CHAN_ATTN i11 = 1)
                fold_wf = pb.raw((B * C * C + (B * C if fold_v else 0),), torch.float32, zero=False)
                fold_bias = fold_wf[B * C * C:] if fold_v else None
                fold_wb = pb.raw((B * C * C,), torch.float32, zero=False)
                fold_sc = pb.raw((B,), torch.float32, zero=False)
                fold_mx = pb.raw((B * (C // 64) * w.groups[s],), torch.float32, zero=False)
            if fold:
                self.fold_stages.append(s)
            for blk in range(w.depths[s]):
                for kind in ("spatial_block", "channel_block"):
                    pre = f"{vt}blocks.{s}.{blk}.{kind}."
                    dwconv_ln(pre + "conv1", pre + "norm1", A_, B_, hbuf)
                    if kind == "spatial_block":
                        linear(pre + "window_attn.qkv", hbuf, qkv)
                        qb = W.f32(pre + "window_attn.qkv.bias")
                        nw = ((H + 11) // 12) ** 2
                        pb.add_op(L.make_op(
                            L.OP_ATTN_ROWS, dt,
                            p=[qkv.ptr, qkv.ptr, qkv.ptr, None, att.ptr, qb.data_ptr() + 4 * C, qb.data_ptr() + 8 * C],
                            i={0: 3 * C, 1: 3 * C, 2: 3 * C, 3: C, 4: 0, 5: C, 6: 2 * C, 7: 0, 8: w.heads[s], 9: 144, 10: 144,
                               11: B * nw, 12: 1, 13: H, 14: H, 15: C // w.heads[s], 16: 1 if (attn_split and grp["dma"]) else 0},
                            f={0: (C // w.heads[s]) ** -0.5}))
                        att.fmt = "split" if (attn_split and grp["dma"]) else "f32"
                        linear(pre + "window_attn.proj", att, B_, res=B_)
                    elif fold:
                        # channel attention folded into its projection (csrc/caption_ops.hip "fold mode"): q|k in f32 for the scores,
                        # v straight into format B (two launches over row slices of the ONE packed q|k|v weight), softmax + fold write
                        # this block's per-image projection weights, and the projection reads v through them — no apply pass, no `att`
                        key = pre + "channel_attn.qkv"
                        wp, _ = W.linear([key], dma=True)
                        wqk, bqk, wv, bv = W.cached((key, dt, "dma-qk|v"), lambda: (
                            pb.weight_rows(wp, 0, 2 * C), pb.upload(sd[key + ".bias"][:2 * C].float()),
                            pb.weight_rows(wp, 2 * C, C), pb.upload(sd[key + ".bias"][2 * C:].float())))
                        assert hbuf.fmt == "split"
                        if scores_in_gemm:
                            # nobody but the scores reads q|k: the launch reduces its tiles to the score partials in its epilogue (rows
                            # ordered [q_g | k_g] per group) and the op below starts at the softmax — no q|k tensor, no scores kernel
                            wqs, bqs = W.cached((key, dt, "dma-qk-groups"), lambda: (
                                pb.pack_weight_qk_groups(wqk), pb.upload(sd[key + ".bias"][:2 * C].float()[pb.qk_group_rows(C)])))
                            pb.conv_scores(tokens(hbuf), wqs, bqs, cws, N)
                        else:
                            pb.conv(tokens(hbuf), wqk, bqk, tokens(qkv.slice(0, 2 * C)), 1)
                        pkey = pre + "channel_attn.proj"
                        chan_p = [qkv.ptr, None, fold_wf.data_ptr(), fold_wb.data_ptr(), None, cws.data_ptr(), fold_sc.data_ptr(), fold_mx.data_ptr()]
                        chan_i = {0: B, 1: N, 3: C, 4: w.groups[s], 5: chunk_tokens, 6: 1 if (attn_split and grp["dma"]) else 0, 8: 1,
                                  9: 1 if scores_in_gemm else 0, 10: partial_tokens}
                        if fold_v:
                            # no v launch: softmax + fold + pack leave W'_b (and b''_b, and 2^-k 2^-kv as the scale), the fold GEMM turns it
                            # into W''_b = W'_b Wv over fold_wf, the re-pack (OMNI_OP_SPLIT_CONVERT i6 = 1) packs that, and the projection reads h itself
                            wvt, wpb = W.cached((key, dt, "dma-vT|wp|bv|bp"), lambda: (
                                pb.pack_weight_dma(sd[key + ".weight"][2 * C:].float().t().contiguous()),
                                pb.upload(torch.cat([sd[pkey + ".weight"].float().reshape(-1), sd[key + ".bias"][2 * C:].float(),
                                                     sd[pkey + ".bias"].float()]))))
                            pb.keep += [wvt, wpb]
                            chan_p[1] = wpb.data_ptr()
                            pb.add_op(L.make_op(L.OP_CHAN_ATTN, dt, p=chan_p, i={**chan_i, 11: 1}, f={1: wvt.omni_oscale}))
                            pb.fold_gemm(fold_wb, fold_sc, wvt, fold_wf, B, C)
                            pb.repack_per_image(fold_wf, fold_wb, fold_sc, fold_mx, B, C)
                            pb.conv_per_image(tokens(hbuf), fold_wb, fold_sc, fold_bias, tokens(B_), tokens(B_), N, bias_per_image=True)
                            pb.flops += 2 * B * N * C * C      # the v layer's algorithmic work: unchanged by no launch running it
                        else:
                            vs = tokens(qkv.slice(2 * C, C))
                            pb.conv(tokens(hbuf), wv, bv, vs, 1, out_split=True)
                            wplain, bproj = W.f32(pkey + ".weight"), W.f32(pkey + ".bias")
                            pb.keep += [wplain, bproj]
                            chan_p[1] = wplain.data_ptr()
                            pb.add_op(L.make_op(L.OP_CHAN_ATTN, dt, p=chan_p, i=chan_i))
                            pb.conv_per_image(vs, fold_wb, fold_sc, bproj, tokens(B_), tokens(B_), N)
                    else:
                        linear(pre + "channel_attn.qkv", hbuf, qkv)
                        pb.add_op(L.make_op(L.OP_CHAN_ATTN, dt, p=[qkv.ptr, None, None, None, att.ptr, cws.data_ptr()],
                                            i={0: B, 1: N, 3: C, 4: w.groups[s], 5: chunk_tokens, 6: 1 if (attn_split and grp["dma"]) else 0}))
                        att.fmt = "split" if (attn_split and grp["dma"]) else "f32"
                        linear(pre + "channel_attn.proj", att, B_, res=B_)
                    dwconv_ln(pre + "conv2", pre + "norm2", B_, A_, hbuf)
                    if mlp_one:
                        k1, k2 = pre + "ffn.fc1", pre + "ffn.fc2"
                        w1p, b1p = W.linear([k1], dma=True)
                        w2p, b2p = W.cached((k2, dt, "dma-kperm"), lambda: (pb.pack_weight_dma(sd[k2 + ".weight"], kperm=True),
                                                                             pb.upload(sd[k2 + ".bias"].float())))
                        pb.mlp_fused(tokens(hbuf), w1p, b1p, w2p, b2p, tokens(A_), tokens(A_))
                        continue
                    linear(pre + "ffn.fc1", hbuf, ffn, act=L.ACT_GELU, out_split=True)
                    linear(pre + "ffn.fc2", ffn, A_, res=A_)
            x = A_
            self.stage_out.append(A_)
            # reuse_activations: the stage's scratch tensors back the (smaller) tensors of the next stages
            pb.release(B_, hbuf, qkv, att, ffn, cws, fold_wf, fold_wb, fold_sc, fold_mx)
        self.vision_out = x
        grp["dma"] = use_dma
        # ---------------- projector
        mp = "model.multi_modal_projector."
        h = x.H
        Cv = x.C

        def pos_tables():
            col = sd[mp + "image_position_embed.column_embeddings.weight"][:h]
            row = sd[mp + "image_position_embed.row_embeddings.weight"][:h]
            pos = torch.cat([col.unsqueeze(0).repeat(h, 1, 1), row.unsqueeze(1).repeat(1, h, 1)], -1).reshape(h * h, Cv)
            return pb.upload(pos.float()), pb.upload(sd[mp + "visual_temporal_embed.pos_idx_to_embed"][0].float())
        pos2d, temporal = W.cached(("pos2d", h), pos_tables)
        pb.keep += [pos2d, temporal]
        n_img = h * h + 1
        self.n_img = n_img
        pp = pb.alloc(B, n_img, 1, Cv)
        pb.add_op(L.make_op(L.OP_PROJ_PREP, dt, p=[x.ptr, pos2d.data_ptr(), temporal.data_ptr(), None, pp.ptr],
                            i={0: B, 1: h * h, 3: Cv}))
        D = w.d_model
        pj = pb.alloc(B, n_img, 1, D)
        linear(mp + "image_projection", pp, pj, bias=False)
        img_feat = pb.alloc(B, n_img, 1, D)
        layernorm(mp + "image_proj_norm", pj, img_feat)
        self.img_feat = img_feat
        if embed:
            # ---------------- embed-only plan set: the op list up to here (the same ops in the same buffers as every caption plan of this
            # capacity), then OMNI_OP_VISUAL_MATCH mode 0 on row 0 of every crop.  No OMNI_OP_ASSEMBLE, no encoder, no cross-K/V, no step plan.
            assert arena is None and not (beam or force or controls or vocab or scores) and n_txt is None
            self.emb = pb.raw((B, D), torch.float32)
            self.emb_norm = pb.raw((B,), torch.float32)
            pb.add_op(embed_op(dt, img_feat.ptr, n_img * D, self.emb, self.emb_norm, B, D))
            self.S = self.prompt_ids = self.nkeys = self.step_plan = self.free_evt = None
            self.cross_kv = []
            self.n_encode_ops = len(pb.ops)
            self.encode_flops = pb.flops
            self.encode_plan = pb.build()
            if dev.type == "cuda":
                torch.cuda.synchronize(dev)         # allocations / uploads ran on the current stream: order them before cap.stream
            if cap.use_graph:
                self.encode_plan.run(cap.stream)    # first launches outside a capture
                cap.stream.synchronize()
                self.encode_plan.capture(cap.stream)
                cap.stream.synchronize()
            return
        # ---------------- encoder
        lm = "model.language_model."
        S = n_img + (len(PROMPT_IDS) if n_txt is None else n_txt)
        self.S = S
        self.prompt_ids = self.nkeys = None
        if n_txt is None:
            txt = W.cached(("prompt", dt), lambda: pb.upload((sd[lm + "shared.weight"][torch.tensor(PROMPT_IDS)] * w.embed_scale).to(torch_dtype(dt))))
            pb.keep.append(txt)
            enc = pb.alloc(B, S, 1, D)
            pb.add_op(L.make_op(L.OP_ASSEMBLE, dt, p=[img_feat.ptr, txt.data_ptr(), None, None, enc.ptr],
                                i={0: B, 1: n_img, 2: len(PROMPT_IDS), 3: D}))
        else:
            table, _ = W.token_tables()
            pb.keep.append(table)
            self.prompt_ids = pb.raw((B, n_txt), torch.int32)
            self.nkeys = pb.raw((B,), torch.int32)
            if arena is None:                      # (a twin shares the arena's two tensors: rows beyond a batch keep valid content)
                self.prompt_ids.fill_(w.pad)
                self.nkeys.fill_(S)
            enc = pb.alloc(B, S, 1, D)
            pb.add_op(L.make_op(L.OP_ASSEMBLE, dt, p=[img_feat.ptr, None, self.prompt_ids.data_ptr(), table.data_ptr(), enc.ptr],
                                i={0: B, 1: n_img, 2: n_txt, 3: D, 4: table.shape[0]}, f={0: w.embed_scale}))
        encpos = W.cached(("encpos", S, dt), lambda: pb.upload(sd[lm + "encoder.embed_positions.weight"][2:2 + S].to(torch_dtype(dt))))
        pb.keep.append(encpos)
        xa = pb.alloc(B, S, 1, D)
        dma_enc = grp["dma"] = use_dma and D % 128 == 0     # every encoder linear (K = D or 4D, N multiple of D) then takes the DMA GEMM
        xs = pb.alloc(B, S, 1, D) if dma_enc else None        # format-B twin of xa (xa itself stays f32: it is the residual)
        layernorm(lm + "encoder.layernorm_embedding", enc, xa, add=encpos, period=S, split=xs)
        xin = xs if dma_enc else xa
        qkv = pb.alloc(B, S, 1, 3 * D)
        att = pb.alloc(B, S, 1, D)
        tmp = pb.alloc(B, S, 1, D)
        ffn = pb.alloc(B, S, 1, sd[lm + "encoder.layers.0.fc1.weight"].shape[0])
        nh = w.n_heads
        for l in range(w.enc_layers):
            pre = f"{lm}encoder.layers.{l}."
            linear(None, xin, qkv, keys=[pre + "self_attn.q_proj", pre + "self_attn.k_proj", pre + "self_attn.v_proj"])
            pb.add_op(L.make_op(L.OP_ATTN_ROWS, dt, p=[qkv.ptr, qkv.ptr, qkv.ptr, None, att.ptr]
                                + ([None, None, self.nkeys.data_ptr()] if self.nkeys is not None else []),
                                i={0: 3 * D, 1: 3 * D, 2: 3 * D, 3: D, 4: 0, 5: D, 6: 2 * D, 7: 0, 8: nh, 9: S, 10: S, 11: B,
                                   12: 0, 15: 64, 16: 1 if (attn_split and dma_enc) else 0}, f={0: 64 ** -0.5}))
            att.fmt = "split" if (attn_split and dma_enc) else "f32"
            linear(pre + "self_attn.out_proj", att, tmp, res=xa)
            layernorm(pre + "self_attn_layer_norm", tmp, xa, split=xs)
            linear(pre + "fc1", xin, ffn, act=L.ACT_GELU, out_split=True)
            linear(pre + "fc2", ffn, tmp, res=xa)
            layernorm(pre + "final_layer_norm", tmp, xa, split=xs)
        self.enc_out = xa
        # ---------------- cross-attention K/V of every decoder layer (computed once per batch)
        self.cross_kv = []
        for l in range(w.dec_layers):
            pre = f"{lm}decoder.layers.{l}.encoder_attn."
            kv = pb.alloc(B, S, 1, 2 * D)
            linear(None, xin, kv, keys=[pre + "k_proj", pre + "v_proj"])
            self.cross_kv.append(kv)
        self.free_evt = None        # recorded behind the last use of this plan's buffers when that was on another stream (parse_stream)
        self.n_encode_ops = len(pb.ops)
        self.encode_flops = pb.flops
        self.encode_plan = pb.build()
        if arena is not None:
            # encode-only twin in the arena's buffers: every kernel of this op list has run before (the arena's own plan warmed it
            # up), nothing was allocated, so the graph is captured straight away on the lane's stream (thread-local capture mode:
            # work in flight on this and other streams is not disturbed, nothing executes here)
            assert len(pb.alloc_log) == len(arena.pb.alloc_log) and self.n_encode_ops == arena.n_encode_ops, \
                "arena replay: the two builds made different allocation / op sequences"
            if cap.use_graph:
                self.encode_plan.capture(stream or cap.stream)
            return
        # ---------------- decoder step plan (for a single micro-batch; batches of several micro-batches decode through _DecodePlans)
        self._build_step(cap, B, max_new, S, self.cross_kv, pb.ws, beam=beam, nkeys=self.nkeys, scores=scores, force=force, controls=controls,
                         vocab=vocab)
        self._warm_up_and_capture(cap, self.encode_plan, self.step_plan)

    def set_prompt(self, ids: torch.Tensor, nkeys: torch.Tensor, n: int):
        """write the prompt of rows [0, n) — ids i32 [n, n_txt] (or [1, n_txt] for all rows), nkeys i32 [n] (or [1]) — on the
        current stream, before the encode plan is replayed (a twin of `encode_rows` reads the same two tensors)"""
        assert self.prompt_ids is not None and ids.shape[-1] == self.n_txt and n <= self.B
        self.prompt_ids[:n].copy_(ids.expand(n, -1), non_blocking=True)
        self.nkeys[:n].copy_(nkeys.expand(n), non_blocking=True)

    def rows_for(self, cap: "Florence2Captioner", n: int) -> int:
        """Row count of the graph a micro-batch of n < B crops runs in this plan set's buffers.  Building a twin costs what building a
        plan costs on the host (~900 op descriptors + a graph capture: a few hundred ms), so a stream whose remainder differs from batch
        to batch must not build one per batch (measured: the mixed-resolution stream fell from 8.1 to 5.8 screenshots/s when every count
        got its own graph).  Policy: a count that is cached, or that the captioner saw for the previous remainder too (a steady load:
        the bench's 89, a service under constant traffic), runs EXACTLY; any other count runs the twin of the next capacity of the
        ladder (8, 16, 32, 64, 96 — at most five twins per plan set, the old bucket plans without their buffers)."""
        last, cap._last_remainder = getattr(cap, "_last_remainder", None), n
        if n in self._row_plans or n == last:
            return n
        return min(cap.bucket(n), self.B)

    def encode_rows(self, cap: "Florence2Captioner", n: int, stream=None) -> "_CaptionPlans":
        """encode-only plan set of exactly n <= B rows in this plan set's buffers (built and captured on first use; the
        `cap.row_graphs` most recently used row counts stay).  The caller issues it on the stream that orders this plan set's uses."""
        assert self.arena is None and 1 <= n <= self.B
        if n == self.B:
            return self
        cp = self._row_plans.pop(n, None)
        if cp is None:
            while len(self._row_plans) >= max(1, int(cap.row_graphs)):
                if dev_sync := (cap.device.type == "cuda"):
                    torch.cuda.synchronize(cap.device)                  # the evicted graph may still be executing (rare: `row_graphs` distinct counts)
                self._row_plans.pop(next(iter(self._row_plans)))
            cp = _CaptionPlans(cap, n, self.R, self.T - 1, arena=self, stream=stream)
            cap.row_graph_builds = getattr(cap, "row_graph_builds", 0) + 1
        self._row_plans[n] = cp                                         # most recently used last
        return cp


# ------------------------------------------------------------------------------------------ public objects
class _Config(SimpleNamespace):
    pass


class Florence2Captioner:
    """Duck-types the `model` half of the reference's caption_model_processor dict
    (ref:util/utils.py:108-125): `.config.name_or_path`, `.config.model_type`, `.device`, `.generate`."""
    # plan composition switches (class attributes: the tests build the round-2 composition by overriding them)
    fuse_dwln = True          # x + dwconv(x) -> LayerNorm as one strip kernel (DaViT stages 0-2)
    attn_split_out = True     # attention kernels write format B for the projection GEMM themselves
    fold_chan_proj = True     # channel attention's apply pass folded into a per-image projection weight where N >= 4 C (f32 LDS-DMA plans;
                              # DaViT stages 0-2 at 768x768, nothing at 64x64): OMNI_OP_CHAN_ATTN i8 = 1 + OMNI_OP_CONV i26 / i27 / p6
    fold_chan_v = True        # folded stages: Wv folded into the per-image projection weight as well — no v launch, the projection reads the
                              # block's LayerNorm output with a per-image bias (OMNI_OP_CHAN_ATTN i11, OMNI_OP_CONV i29)
    chan_scores_in_gemm = True   # folded stages: the q|k launch reduces its tiles to the score partials in its epilogue (OMNI_OP_CONV i28 / p7)
                              # and OMNI_OP_CHAN_ATTN starts at the softmax (i9 = 1); off: plain q|k launch + the standalone scores kernel
                              # over the same 256-token chunks — bit-identical results (the A/B and test switch)
    fuse_mlp = True           # fc1 + GELU + fc2 + residual of the C = 128 stage as ONE kernel (OMNI_OP_MLP_FUSED): no hidden tensor in HBM
    exact_rows = os.environ.get("OMNI_EXACT_ROWS", "1") != "0"   # merged decode: the remainder micro-batch of a caption batch encodes exactly
                              # its own rows, as a second hipGraph over the buffers of the lane's full-capacity plan (`_CaptionPlans.encode_rows`),
                              # instead of a padded bucket plan with its own activations; `row_graphs` such graphs stay per plan set
    row_graphs = int(os.environ.get("OMNI_CAPTION_ROW_GRAPHS", "24"))
    patch_rows = os.environ.get("OMNI_PATCH_ROWS", "1") != "0"   # first patch embedding in row-patch form on the split-f16 kernel (f32 plans)
    reuse_activations = True  # scratch tensors of a DaViT stage are released at its end and back the tensors of the later stages
                              # (PlanBuilder.release): same kernels, same order, different addresses — a rank's plan sets hold 89 GB
                              # instead of 176 GB of HBM at the same speed (profiles/r4_s2_candidates_ab.txt).  With it `stage_out[:3]` are
                              # no longer valid after the encode plan: the bisection taps (tools/archive/r3_bisect.py) turn it off

    long_kv_budget_bytes = 2 ** 30   # `generate` / `caption_crops`: the self-attention K / V of one plan (rows x T x d_model x 4 B x 2 x
                              # decoder layers; 165 MB at 128 rows and T = 35, 4.8 GB at T = 1025) stays under this: longer outputs
                              # run in chunks of fewer rows (`long_plan_rows`)

    def __init__(self, model_dir, device=None, precision: Optional[str] = None, resolution: Optional[int] = None):
        device = L.require_device(device, "Florence2Captioner")
        L.lib()
        self.device = device
        precision = precision or os.environ.get("OMNI_PRECISION", "f32")
        self.dtype = L.F32 if precision == "f32" else L.F16
        # 768 = the reference's CPU-path crop resolution (parity target); 64 = its cuda branch (do_resize=False)
        self.resolution = int(resolution or os.environ.get("OMNI_CAPTION_RES", "768"))
        self.w = FlorenceWeights(model_dir)
        self.config = _Config(name_or_path=str(model_dir) if "florence" in str(model_dir).lower() else f"florence:{model_dir}",
                              model_type="florence2")
        self.use_graph = os.environ.get("OMNI_HIPGRAPH", "1") != "0"    # read when a plan is built: tools set the attribute to profile eagerly
        self.stream = self._lane_stream(0)
        self._wcache = {}
        self._plans = {}
        self.max_new_tokens = 20
        self.early_exit_every = 5        # poll the all-rows-finished flag every N decode steps (0 = always run max_new_tokens steps)
        self.num_beams = 1               # caption_crops / ScreenParser: 1 = greedy (the reference's call), k > 1 = beam search
        self.token_scores = False        # caption_crops / ScreenParser: also return the greedy tokens' log-probabilities / a confidence
        self.last_steps = 0              # decode steps the last `_run` / `_decode_merged` issued
        self._lut, self._bic = None, {}  # crop op tables (`_crop_tables`)
        self._lock = L.DeviceLock(self.device, reentrant=True)   # one caption batch at a time per model; makes this GPU the thread's current device

    def to(self, *a, **k):
        return self

    def eval(self):
        return self

    @staticmethod
    def bucket(n: int) -> int:
        """plan capacity for a micro-batch of n crops (rows beyond n are computed and ignored): powers of two plus 96 — the bench
        step's 349 crops are 128 + 128 + 93, and a 96-row plan for that tail computes 8 % fewer rows per step than a third 128-row
        one.  Every capacity is one more resident plan (~25 GB of activations at 128 rows, 768x768 crops — 60 GB without activation reuse; at most OMNI_CAPTION_PLAN_GB
        stay resident), which is why the ladder is not finer; OMNI_CAPTION_BUCKETS overrides it."""
        for b in _BUCKETS:
            if n <= b:
                return b
        return _BUCKETS[-1]

    # ---- long outputs
    def max_new_limit(self) -> int:
        """largest max_new_tokens: the decoder step of generated position p reads row p + 2 of the learned position table"""
        return int(self.w.sd["model.language_model.decoder.embed_positions.weight"].shape[0]) - 2

    def check_max_new(self, max_new_tokens, beam=None) -> int:
        """max_new_tokens of `generate` / `caption_crops` / `plans`, or a ValueError naming the limit: an int in 1..rows of the
        decoder position table - 2; with beam search (beam = `beam_config`) also what OMNI_OP_BEAM_STEP's LDS staging holds."""
        lim, why = self.max_new_limit(), "the decoder's position table has no row beyond that"
        if beam and beam_max_new(beam[0]) < lim:
            lim, why = beam_max_new(beam[0]), f"beam search with num_beams={beam[0]} stages every position of its beams in LDS"
        n = max_new_tokens
        if isinstance(n, bool) or not isinstance(n, int) or n < 1 or n > lim:
            raise ValueError(f"max_new_tokens must be an integer in 1..{lim} ({why}), got {n!r}")
        return n

    def long_plan_rows(self, max_new_tokens: int, k: int = 1) -> int:
        """crops per plan for outputs of max_new_tokens: the largest capacity of the bucket ladder whose self-attention K / V
        (k decoder rows per crop) stays within `long_kv_budget_bytes`, at least the smallest capacity.  128 up to T = 227."""
        per_row = (int(max_new_tokens) + 1) * self.w.d_model * 4 * 2 * self.w.dec_layers * max(int(k), 1)
        fit = [b for b in _BUCKETS if b * per_row <= self.long_kv_budget_bytes]
        return fit[-1] if fit else _BUCKETS[0]

    @staticmethod
    def decode_bucket(n: int) -> int:
        """row capacity of the merged decode plan for n crops: multiples of 32 (the unused tail rows are computed and ignored).  Rounds
        3-5 rounded to 128: at the benched load (345 crops) that decoded 384 rows, i.e. 11 % of every per-row decode kernel —
        cross-attention streams 21.6 MB of K / V per row and step — was padding (50.4 vs 48.0 ms per batch measured in
        round 3's probe).  The micro-batches copy exactly their own n rows into the plan (`_encode_into`), so any capacity >= n works;
        32 keeps the number of distinct plans (8 GB each at 384 rows) small on a stream with varying crop counts."""
        return max(128, (n + 31) // 32 * 32)

    # ---- resident plan sets: ONE cache for encode and decode plans, bounded by BYTES (and, secondarily, by count), LRU, never
    # evicting what the batch being issued has already taken.  A 128-row plan set at 768x768 crops holds ~25 GB of activations (60 GB without activation reuse), a
    # 384-row decode plan ~8 GB: a bound counted in plans either thrashes on a stream with varying crop counts (every eviction is a
    # device-wide synchronise + a rebuild of tens of GB + a graph capture) or lets the resident set grow past the HBM.
    def begin_batch(self):
        """Called by the pipeline before it takes the plans of one caption batch: everything taken from here on is pinned until the
        next call (at most 2 lane plans + 1 remainder plan + 1 decode plan)."""
        self._epoch = getattr(self, "_epoch", 0) + 1

    def _wcache_bytes(self) -> int:
        """device bytes of the packed weights shared by all plans of this model (tensors, or tuples of tensors / None)"""
        n = 0
        for v in self.__dict__.get("_wcache", {}).values():
            for t in (v if isinstance(v, (tuple, list)) else (v,)):
                if isinstance(t, torch.Tensor):
                    n += t.numel() * t.element_size()
        return n

    def plan_cache_bytes(self) -> int:
        return sum(m[0] for k, m in self.__dict__.get("_plan_meta", {}).items() if k in self._plans)

    def clear_plans(self):
        """drop every resident plan set (the caller has synchronised the captioner's streams)"""
        self._plans.clear()
        self.__dict__.get("_plan_meta", {}).clear()

    def _cached_plan(self, key, build):
        meta = self.__dict__.setdefault("_plan_meta", {})
        epoch = getattr(self, "_epoch", 0)
        if key in self._plans:
            self._plans[key] = self._plans.pop(key)            # most recently used last
            meta.setdefault(key, [0, epoch])[1] = epoch        # (an entry placed in _plans from outside has no record: size unknown)
            return self._plans[key]
        max_bytes = int(float(os.environ.get("OMNI_CAPTION_PLAN_GB", "200")) * 2 ** 30)
        max_plans = int(os.environ.get("OMNI_MAX_CAPTION_PLANS", "16"))
        base = key[:4] if key[0] == "dec" else key[:3]         # the key without its slot: twins have the same size
        sizes = self.__dict__.setdefault("_plan_sizes", {})    # bytes of every plan set ever built (survives eviction): the estimate
        est = sizes.get(base, 0)                               # for the one about to be built
        if not est and sizes:
            # a shape never built before: scale the bytes-per-row of the known shape of the same kind and resolution (activations are
            # linear in the row count) — so the byte bound also guards FIRST builds of non-default buckets / lanes / resolutions
            same = [(b, v) for b, v in sizes.items() if (b[0] == "dec") == (base[0] == "dec") and b[-2] == base[-2] and v]
            if same:
                b0, v0 = max(same, key=lambda bv: bv[1])
                rows0, rows = (b0[1] if b0[0] == "dec" else b0[0]), (base[1] if base[0] == "dec" else base[0])
                est = int(v0 * rows / max(rows0, 1))
        def over():
            return len(self._plans) >= max_plans or (self._plans and self.plan_cache_bytes() + est > max_bytes)
        while over():
            victim = next((k for k in self._plans if meta.get(k, [0, None])[1] != epoch), None)
            if victim is None:
                break                                          # everything resident belongs to the batch being issued
            torch.cuda.synchronize(self.device)                # work of any of the captioner's streams may still use the evicted plan's buffers
            self._plans.pop(victim)
            meta.pop(victim, None)
            self.plan_evictions = getattr(self, "plan_evictions", 0) + 1
            L.gc_after_eviction()
        on_gpu = self.device.type == "cuda" and torch.cuda.is_available()
        before = torch.cuda.memory_allocated(self.device) if on_gpu else 0
        w_before = self._wcache_bytes()
        import contextlib
        with (torch.cuda.device(self.device) if self.device.type == "cuda" else contextlib.nullcontext()):
            obj = build()
        self._plans[key] = obj
        # the plan's OWN bytes: the first build of a model also uploads the shared weights (the weight cache outlives every plan and
        # is not freed by an eviction), which must not be booked on whichever plan happened to come first
        grown = (torch.cuda.memory_allocated(self.device) if on_gpu else 0) - before - (self._wcache_bytes() - w_before)
        meta[key] = [max(0, grown), epoch]
        sizes[base] = meta[key][0]
        return obj

    def beam_config(self, num_beams=None, length_penalty=None, early_stopping=None):
        """(k, length_penalty, early_stopping) of a beam plan, or None for greedy decoding; unset values come from the checkpoint's
        generation settings (FlorenceWeights)."""
        k = self.num_beams if num_beams is None else num_beams
        if isinstance(k, bool) or not isinstance(k, int) or k < 1 or k > BEAM_MAX:
            raise ValueError(f"num_beams must be an integer in 1..{BEAM_MAX} (got {k!r})")
        if k == 1:
            return None
        lp = float(self.w.length_penalty if length_penalty is None else length_penalty)
        es = check_early_stopping(self.w.early_stopping if early_stopping is None else early_stopping)
        return (k, lp, es)

    @torch.inference_mode()
    def decode_plans(self, B, R, max_new, slot=0, beam=None, n_txt=None, scores=False, vocab=False) -> _DecodePlans:
        """slot: the pipelined stream (pipeline.py::parse_stream) decodes batch i on its own HIP stream while batch i+1 encodes, so it
        alternates between two decode plans (8 GB of cross-attention K/V each at 384 rows, 768x768 crops).  beam: see
        `beam_config` (B crops = B k decoder rows).  n_txt: text capacity of a batch with a prompt (`prompt_batch`).  vocab (greedy
        only): the plan that ends in OMNI_OP_GREEDY_VOCAB_STEP (`plans`); part of the cache key."""
        self.check_max_new(max_new, beam)
        if vocab and beam:
            raise ValueError("a closed vocabulary is applied by greedy decoding only (no beam search)")
        key = ("dec", B, R, max_new) if slot == 0 else ("dec", B, R, max_new, slot)
        if beam or n_txt is not None:
            key = ("dec", B, R, max_new, slot, beam) + (() if n_txt is None else (("txt", n_txt),))
        if scores:                     # token log-probabilities (greedy): a plan set of its own, like a beam configuration
            key = ("dec", B, R, max_new, slot, beam) + (() if n_txt is None else (("txt", n_txt),)) + ("scores",)
        if vocab:
            key = ("dec", B, R, max_new, slot, None) + (() if n_txt is None else (("txt", n_txt),)) + (("scores",) if scores else ()) + ("vocab",)
            return self._cached_plan(key, lambda: _DecodePlans(self, B, R, max_new, n_txt=n_txt, scores=scores, vocab=True))
        return self._cached_plan(key, lambda: _DecodePlans(self, B, R, max_new, beam=beam, n_txt=n_txt, scores=scores))

    @torch.inference_mode()
    def plans(self, B, R, max_new, slot=0, beam=None, n_txt=None, scores=False, force=None, controls=False, vocab=False) -> _CaptionPlans:
        """slot 1 = a second, independent set of buffers of the same capacity: the pipelined stream (pipeline.py::parse_stream) keeps two
        128-crop micro-batches in flight on two HIP streams (~25 GB of activations each at 768x768 with activation reuse, 60 GB without).
        beam: see `beam_config` (the step plan decodes B k rows).  n_txt: text capacity of a batch with a prompt (`prompt_batch`);
        it is part of the cache key, None = the default prompt's plan.  controls (greedy only): the plan that ends in
        OMNI_OP_GREEDY_CTRL_STEP and owns a control block (`_StepPlans.set_controls`); part of the cache key beside `scores`, and
        only ever built by a call with non-neutral `GenerationControls` — one plan serves every setting.  vocab (greedy only, no
        controls): the plan that ends in OMNI_OP_GREEDY_VOCAB_STEP and owns the rows' trie nodes and a trie buffer
        (`_StepPlans.set_vocabulary`); part of the cache key beside `scores` and `controls`, only ever built by a call with a
        `CaptionVocabulary` — one plan and graph serve every vocabulary."""
        self.check_max_new(max_new, beam)
        if vocab and (beam or force or controls):
            raise ValueError("a closed vocabulary is applied by greedy decoding only (no beam search, no teacher-forced scoring, no "
                             "generation controls)")
        if controls and (beam or force):
            raise ValueError("generation controls are applied by greedy decoding only (no beam search, no teacher-forced scoring)")
        key = (B, R, max_new) if slot == 0 else (B, R, max_new, slot)
        if beam or n_txt is not None:
            key = (B, R, max_new, slot, beam) + (() if n_txt is None else (("txt", n_txt),))
        if scores:
            key = (B, R, max_new, slot, beam) + (() if n_txt is None else (("txt", n_txt),)) + ("scores",)
        if force:                      # teacher-forced scoring of `force` candidate rows per crop, max_new = the label capacity
            key = (B, R, max_new, slot, None) + (() if n_txt is None else (("txt", n_txt),)) + (("force", force, max_new),)
            return self._cached_plan(key, lambda: _CaptionPlans(self, B, R, max_new, n_txt=n_txt, force=force))
        if controls:
            key = (B, R, max_new, slot, None) + (() if n_txt is None else (("txt", n_txt),)) + (("scores",) if scores else ()) + ("controls",)
            return self._cached_plan(key, lambda: _CaptionPlans(self, B, R, max_new, n_txt=n_txt, scores=scores, controls=True))
        if vocab:
            key = (B, R, max_new, slot, None) + (() if n_txt is None else (("txt", n_txt),)) + (("scores",) if scores else ()) + ("vocab",)
            return self._cached_plan(key, lambda: _CaptionPlans(self, B, R, max_new, n_txt=n_txt, scores=scores, vocab=True))
        return self._cached_plan(key, lambda: _CaptionPlans(self, B, R, max_new, beam=beam, n_txt=n_txt, scores=scores))

    @torch.inference_mode()
    def embed_plans(self, B, R) -> _CaptionPlans:
        """the embed-only plan set of B crops at resolution R (`_CaptionPlans(embed=True)`): an entry of the plan cache of its own
        (`embed` is in the key, which no caption plan's key holds), under the same byte-bounded LRU; only ever built by `embed` /
        `embed_crops`"""
        return self._cached_plan((B, R, 0, 0, None, "embed"), lambda: _CaptionPlans(self, B, R, 1, embed=True))

    def generation_controls(self, controls, max_new_tokens, beam=None) -> Optional[GenerationControls]:
        """`controls` (None, a dict of GEN_CTRL_KEYS or a GenerationControls) checked against this model, before anything touches a
        device: None when they are neutral (the call is the default call), else the checked object.  ValueError: a bad value
        (`GenerationControls`, `GenerationControls.check`), or non-neutral controls together with beam search — transformers applies
        the processors to log-probabilities there, which OMNI_OP_BEAM_STEP does not do."""
        gc = GenerationControls.of(controls).check(self.w.vocab, max_new_tokens, self.w.eos, self.w.forced_bos, self.w.forced_eos)
        if gc.neutral:
            return None
        if beam:
            raise ValueError("generation controls (repetition_penalty, no_repeat_ngram_size, min_new_tokens, suppress_tokens, "
                             "begin_suppress_tokens, bad_words_ids) are not supported with beam search (num_beams > 1): greedy decoding only")
        return gc

    def caption_vocabulary(self, vocabulary, max_new_tokens, beam=None, controls=None) -> Optional[CaptionVocabulary]:
        """`vocabulary` (None, a list of labels as id lists, or a CaptionVocabulary) checked against this model, before anything
        touches a device: None when there is none, else the checked object.  ValueError: a bad label (`CaptionVocabulary`,
        `CaptionVocabulary.check`), or a vocabulary together with beam search or with non-neutral generation controls (`controls`:
        what `generation_controls` returned) — neither path reads the trie."""
        if vocabulary is None:
            return None
        if beam:
            raise ValueError("a closed vocabulary (vocabulary=...) is not supported with beam search (num_beams > 1): greedy decoding only")
        if controls is not None:
            raise ValueError("a closed vocabulary (vocabulary=...) is not supported together with generation controls (repetition_penalty, "
                             "no_repeat_ngram_size, min_new_tokens, suppress_tokens, begin_suppress_tokens, bad_words_ids)")
        w = self.w
        return CaptionVocabulary.of(vocabulary).check(w.vocab, max_new_tokens, w.eos, w.forced_bos, w.forced_eos, w.ngram, w.start)

    # ---- prompts
    def prompt_batch(self, rows, R):
        """The caller's prompts as plan inputs.  rows: one list of token ids per image (bos ... eos, no padding).  Returns None when
        every row is the default prompt PROMPT_IDS — such a batch runs the plan it always ran, at no cost — else
        (ids i32 [n, n_txt] right-padded with the pad token, valid encoder keys i32 [n] = n_img + length, n_txt) on the host, n_txt
        the smallest of TEXT_CAPACITIES that holds the longest row.  ValueError: an empty prompt, more than 64 tokens (plans at
        768x768 are several GB each, so the capacity ladder stops there), an id outside the token table (refused here: the kernel
        must not be the one to find out)."""
        rows = [[int(t) for t in r] for r in rows]
        if all(r == PROMPT_IDS for r in rows):
            return None
        vocab = self.w.sd["model.language_model.shared.weight"].shape[0]
        for r in rows:
            if not r:
                raise ValueError("an empty prompt: at least one token is needed")
            bad = [t for t in r if not 0 <= t < vocab]
            if bad:
                raise ValueError(f"prompt token id {bad[0]} is outside the token table (0..{vocab - 1})")
        n_txt = text_capacity(max(len(r) for r in rows))
        n_img = (R // 32) ** 2 + 1
        ids = torch.full((len(rows), n_txt), int(self.w.pad), dtype=torch.int32)
        for b, r in enumerate(rows):
            ids[b, :len(r)] = torch.tensor(r, dtype=torch.int32)
        nkeys = torch.tensor([n_img + len(r) for r in rows], dtype=torch.int32)
        return ids, nkeys, n_txt

    def _prompt_from_input_ids(self, input_ids, attention_mask, n, R):
        """`prompt_batch` of generate()'s input_ids [n, n_img + L] (+ attention_mask of the same shape)"""
        if input_ids is None:
            if attention_mask is not None:
                raise ValueError("attention_mask without input_ids")
            return None
        ids = torch.as_tensor(input_ids).detach().cpu().long()
        n_img = (R // 32) ** 2 + 1
        img_tok = int(self.w.cfg.get("image_token_id", 51289))
        if ids.dim() != 2 or ids.shape[0] != n:
            raise ValueError(f"input_ids must be [batch, tokens] with one row per image ({n}), got {tuple(ids.shape)}")
        if ids.shape[1] <= n_img or not bool((ids[:, :n_img] == img_tok).all()):
            raise ValueError(f"input_ids must start with the {n_img} image placeholder tokens (id {img_tok}) of a {R}x{R} image, "
                             "followed by the prompt")
        txt = ids[:, n_img:]
        if attention_mask is None:
            lens = [txt.shape[1]] * n
        else:
            m = torch.as_tensor(attention_mask).detach().cpu()
            if tuple(m.shape) != tuple(ids.shape):
                raise ValueError(f"attention_mask {tuple(m.shape)} does not match input_ids {tuple(ids.shape)}")
            m = m != 0
            if not bool(m[:, :n_img].all()):
                raise ValueError("attention_mask hides image tokens: only prompt padding can be masked")
            mt = m[:, n_img:]
            lens = mt.sum(1).tolist()
            if not bool((mt == (torch.arange(txt.shape[1])[None, :] < mt.sum(1)[:, None])).all()):
                raise ValueError("attention_mask must be right-padded (ones, then zeros): left padding and holes are not supported")
        return self.prompt_batch([txt[b, :lens[b]].tolist() for b in range(n)], R)

    # ---- merged decode (several micro-batches): encode only, cross-KV into rows [row0, row0 + n) of the decode plan
    def _encode_into(self, cp: _CaptionPlans, n: int, dec: _DecodePlans, row0: int, stream=None):
        """encode on `stream` (default: the captioner's first stream; the caller made it current)."""
        stream = stream or self.stream
        assert cp.n_txt == dec.n_txt, "the micro-batches and their merged decode plan have one text capacity"
        if dec.nkeys is not None:
            dec.nkeys[row0:row0 + n].copy_(cp.nkeys[:n], non_blocking=True)
        if n < cp.B and self.exact_rows:
            cp = cp.encode_rows(self, cp.rows_for(self, n), stream)     # n rows (or the ladder capacity above n) in cp's buffers; cross_kv
                                                                        # below: the first n rows of the same tensors
        (cp.encode_plan.replay if self.use_graph else cp.encode_plan.run)(stream)
        for src, dst in zip(cp.cross_kv, dec.cross_kv):
            dst.t[row0:row0 + n].copy_(src.t[:n], non_blocking=True)

    def _decode_merged(self, dec: _DecodePlans, n: int, max_new: int, stream=None) -> torch.Tensor:
        """the 20 decode steps over all rows of `dec` on `stream` (default: the captioner's stream; the caller made it current)."""
        stream = stream or self.stream
        run = dec.step_plan.replay if self.use_graph else dec.step_plan.run
        for _ in range(max_new):
            run(stream)
        self.last_steps = max_new
        return dec.snapshot(n)                     # stream-ordered snapshot (read back by the caller); (ids, logp) from a scores plan

    def _lane_stream(self, k):
        # Measured and not kept (round 4, profiles/r4_s2_candidates_ab.txt): CU-masked lane streams (hipExtStreamCreateWithCUMask) and a
        # two-stream replay with the GEMMs on one CU set and the HBM-bound kernels on the other — 754-1079 ms per bench step against
        # 692 on plain streams, for every partition tried.
        return torch.cuda.Stream(device=self.device)

    @property
    def stream2(self):
        """second encode lane of the pipelined stream: while one 128-crop micro-batch is in its MFMA-bound GEMMs the other one's
        HBM-bound kernels (depthwise conv + LayerNorm, attention, short-K GEMMs) fill the wave slots the GEMM blocks leave free."""
        if getattr(self, "_stream2", None) is None:
            self._stream2 = self._lane_stream(1)
        return self._stream2

    def encode_lane(self, k):
        """stream of encode lane k: 0 / 1 = `stream` / `stream2` (the default pipeline's two lanes); further lanes on demand."""
        if k == 0:
            return self.stream
        if k == 1:
            return self.stream2
        extra = self.__dict__.setdefault("_extra_lanes", {})
        if k not in extra:
            extra[k] = self._lane_stream(k)
        return extra[k]

    @property
    def dec_stream(self):
        """second HIP stream of the captioner: decode steps of batch i (launch-bound GEMMs over a few hundred rows + the HBM-bound
        cross-attention) overlap the MFMA-bound encode of batch i+1 (pipeline.py::parse_stream)."""
        if getattr(self, "_dec_stream", None) is None:
            self._dec_stream = self._lane_stream(2)
        return self._dec_stream

    # ---- decode loop shared by both entry points
    def _run(self, cp: _CaptionPlans, n: int, max_new: int, defer: bool = False, embeds: Optional[list] = None, after=None) -> torch.Tensor:
        run = (lambda p: p.replay(self.stream)) if self.use_graph else (lambda p: p.run(self.stream))
        run(cp.encode_plan)
        if embeds is not None:             # caption_crops(return_embeddings=True): one eager launch behind the encode plan, same stream
            embeds.append(self._embed_rows(cp, n))
        poll = 0 if defer else self.early_exit_every
        steps = 0
        for t in range(max_new):
            run(cp.step_plan)
            steps += 1
            # hf stops as soon as every row has emitted EOS (generation/utils.py:2936) — beam search: as soon as no crop's finished
            # hypotheses can change (`finished` = frozen flags): poll the device flags every few steps (a 4-byte read-back) instead of
            # always paying max_new steps; the deferred (batched-stream) path never syncs
            if poll and (t + 1) % poll == 0 and t + 1 < max_new and bool(cp.finished[:n].min().item()):
                break
        self.last_steps = steps
        if after is not None:              # read_regions: its launches go behind the last step on the same stream; nothing is read back here
            return after(cp, n)
        if defer:                          # stream-ordered snapshot; the caller reads it back later (no sync here)
            return cp.snapshot(n)
        if cp.beam:                        # finished hypotheses [n, k, T], their scores and generated lengths (synchronises)
            return cp.fin_ids[:n].cpu().long(), cp.fin_score[:n].cpu().clone(), cp.fin_len[:n].cpu().long()
        if cp.logp is not None:            # (ids, token log-probabilities) of a scores plan
            return cp.ids[:n].cpu().long(), cp.logp[:n].cpu().clone()
        return cp.ids[:n].cpu().long()     # synchronises the stream

    def _finish_ids(self, ids: torch.Tensor) -> torch.Tensor:
        n = ids.shape[0]
        # hf stops as soon as every row has emitted EOS (generation/utils.py:2936): trim the all-pad tail
        T = ids.shape[1]
        done_at = T
        seen = torch.zeros(n, dtype=torch.bool)
        for t in range(1, T):
            seen |= ids[:, t] == self.w.eos
            if bool(seen.all()):
                done_at = t + 1
                break
        return ids[:, :done_at]

    @torch.inference_mode()
    def generate(self, input_ids=None, pixel_values=None, max_new_tokens=20, num_beams=1, do_sample=False, num_return_sequences=1,
                 length_penalty=None, early_stopping=None, return_dict_in_generate=False, attention_mask=None,
                 repetition_penalty=None, no_repeat_ngram_size=None, min_new_tokens=None, suppress_tokens=None,
                 begin_suppress_tokens=None, bad_words_ids=None, vocabulary=None, **kw):
        """hf-compatible entry point (ref:util/utils.py:125).  pixel_values: [B,3,R,R] float (NCHW).

        input_ids [B, n_img + L]: the first n_img = (R / 32)^2 + 1 columns must be the image placeholder token (anything else is a
        ValueError, not a guess), the rest is the prompt, right-padded when rows differ in length, with an attention_mask of the
        same shape that is 1 on the image columns and on each row's prompt (left padding is a ValueError).  WITHOUT attention_mask
        EVERY column counts — transformers would infer a mask from pad ids when pad != eos; here a pad id without a mask is a
        prompt token.  Up to 64 prompt tokens (`text_capacity`).  input_ids=None, or rows that all equal PROMPT_IDS: the default
        <CAPTION> prompt, on the plan it always ran on.  Works with num_beams > 1 as well.

        num_beams = 1: greedy decoding (the reference's call).  num_beams = 2..8: beam search on the device, transformers'
        `_beam_search` step for step (OMNI_OP_BEAM_STEP); `num_return_sequences` best hypotheses per image (image-major rows),
        `length_penalty` / `early_stopping` default to the checkpoint's generation settings.  return_dict_in_generate=True returns
        an object with `.sequences` and `.sequences_scores` (hf's beam scores; None for greedy decoding).  The default stays
        num_beams=1 although transformers would take num_beams=3 from Florence-2's generation config: changing it would change what
        existing callers get.  Sampling is not implemented.

        output_scores=True (greedy decoding, with return_dict_in_generate=True): the returned object gains `.token_logprobs`, f32
        [B, sequences.shape[1] - 1] aligned with sequences[:, 1:] — the log-probability of every generated token under the processed
        scores, what transformers' compute_transition_scores(sequences, scores, normalize_logits=True) returns for its greedy
        `scores`; 0 at forced positions and behind a row's EOS.  It is computed on the device next to the arg-max (OMNI_OP_GREEDY_STEP
        p4).  hf's `scores` tuple itself (a [B, vocab] tensor per step) is NOT produced: `.scores` does not exist.  With
        num_beams > 1 it is a ValueError — beam search returns `sequences_scores`.

        Generation controls (greedy decoding; each None = not set, as in transformers): repetition_penalty (float > 0; applied once
        to every token of the history, the decoder start token included), no_repeat_ngram_size (int >= 0, 0 = off; None = the
        checkpoint's), min_new_tokens (0..max_new_tokens: no EOS before), suppress_tokens, begin_suppress_tokens (first generated
        position; the second one behind a forced BOS, as in transformers), bad_words_ids (up to 64 sequences of 2..8 tokens, any
        number of single tokens).  They are transformers' processors of the same names in transformers' order, applied on the
        device by OMNI_OP_GREEDY_CTRL_STEP: token ids equal transformers' on the CPU, and `token_logprobs` are those of the
        processed scores.  The block of values is uploaded per call; every setting replays the same plan and graph, and a call
        without controls (or with neutral ones: penalty 1.0, min_new_tokens 0, empty lists) runs the plans it always ran.
        ValueError before anything reaches the device: a value outside its range, a token id outside the vocabulary, the EOS /
        forced BOS / forced EOS token in suppress_tokens, begin_suppress_tokens or as a single-token bad word, and any non-neutral
        control together with num_beams > 1.  Not supported: min_length, sequence_bias, the encoder-side processors, sampling.

        vocabulary (greedy decoding): a closed set of captions — a list of labels, each a list of token ids as
        `FlorenceProcessor.prompt_ids` returns them ([forced BOS] text EOS), or a `CaptionVocabulary`.  Every returned row is then
        the decoder start token + exactly one label + padding: what transformers' generate(prefix_allowed_tokens_fn=fn) returns
        when fn walks the trie of the labels, computed on the device by OMNI_OP_GREEDY_VOCAB_STEP, which reads the trie from device
        memory (one plan and graph for every vocabulary; thousands of labels cost one decode).  With output_scores the
        `token_logprobs` are log-softmax values over the allowed continuations (0 where only one is left), so their sum is the
        label's log-probability among the labels.  return_dict_in_generate=True adds `.label_index` i64 [B]: the label's index
        in the deduplicated vocabulary (`CaptionVocabulary.labels`), -1 for a row that ended outside it (degenerate logits only).
        Works with a caller's prompt and any max_new_tokens from the longest label up.  ValueError before anything reaches the
        device: a label that is empty, longer than 64 tokens, not ending in EOS, holding EOS elsewhere, not starting with the
        forced BOS, with an id outside the vocabulary, a trie of more than 65536 nodes, max_new_tokens below the longest label, a
        prefix whose continuations the checkpoint's no_repeat_ngram_size all bans, and a vocabulary together with num_beams > 1 or
        with any non-neutral generation control (an explicit no_repeat_ngram_size included).  vocabulary=None is the call as it was.
        The `prefix_allowed_tokens_fn` keyword itself is part of **kw and IGNORED: a Python callable cannot run inside a captured
        step graph on the device — pass the set of labels as `vocabulary` instead.

        Any OTHER keyword argument (**kw) is accepted and IGNORED, as it always was: transformers callers pass use_cache,
        output_attentions and the like, which change nothing here.
        """
        if do_sample:
            raise NotImplementedError("sampling is not implemented (greedy or beam search decoding)")
        output_scores = kw.pop("output_scores", False)
        if not isinstance(output_scores, bool):
            raise ValueError(f"output_scores must be a bool, got {output_scores!r}")
        if output_scores and not return_dict_in_generate:
            raise ValueError("output_scores=True needs return_dict_in_generate=True (the scores are a member of the returned object)")
        beam = self.beam_config(num_beams, length_penalty, early_stopping)
        if output_scores and beam:
            raise ValueError("output_scores=True is a greedy-decoding output (num_beams=1); beam search returns sequences_scores")
        self.check_max_new(max_new_tokens, beam)
        controls = self.generation_controls(dict(zip(GEN_CTRL_KEYS, (repetition_penalty, no_repeat_ngram_size, min_new_tokens,
                                                                     suppress_tokens, begin_suppress_tokens, bad_words_ids))),
                                            max_new_tokens, beam)
        vocab = self.caption_vocabulary(vocabulary, max_new_tokens, beam, controls)
        k = beam[0] if beam else 1
        if isinstance(num_return_sequences, bool) or not isinstance(num_return_sequences, int) or not 1 <= num_return_sequences <= k:
            raise ValueError(f"num_return_sequences must be in 1..num_beams ({k}), got {num_return_sequences!r}")
        with self._lock:
            Bn, _, R, R2 = pixel_values.shape
            assert R == R2
            prompt = self._prompt_from_input_ids(input_ids, attention_mask, Bn, R)

            def fill(cp, s, n):
                cp.x_in.t[:n, :, :, :3] = pixel_values[s:s + n].to(self.device).permute(0, 2, 3, 1).to(cp.x_in.t.dtype)
            parts = self._caption_chunks(pixel_values, Bn, 128, R, max_new_tokens, beam, fill, prompt, output_scores, controls, vocab)
            extra = {"label_index": self.label_indices(vocab, parts, output_scores)} if vocab else {}
            if output_scores:
                seq, logp = self._results_scores(parts)
                return SimpleNamespace(sequences=seq, sequences_scores=None, token_logprobs=logp, **extra)
            seq, scores = self._results(parts, beam, num_return_sequences)
        return SimpleNamespace(sequences=seq, sequences_scores=scores, **extra) if return_dict_in_generate else seq

    def label_indices(self, vocab: CaptionVocabulary, parts, scores=False) -> torch.Tensor:
        """i64 [n]: per row of the per-chunk greedy `_run` results the index of the label it spells in `vocab.labels`, -1 for none"""
        rows = [r for p in parts for r in (p[0] if scores else p)[:, 1:].tolist()]
        return torch.tensor([vocab.label_index(r, self.w.eos) for r in rows], dtype=torch.long)

    def _embed_rows(self, cp: _CaptionPlans, n: int) -> torch.Tensor:
        """f32 [n, D] on the device: OMNI_OP_VISUAL_MATCH mode 0 on row 0 of the first n crops of `cp.img_feat`, launched eagerly on
        the captioner's stream behind the encode plan that wrote it (img_feat is never released to another tensor of the plan)"""
        D = self.w.d_model
        out = torch.empty((n, D), dtype=torch.float32, device=self.device)
        norm = torch.empty((n,), dtype=torch.float32, device=self.device)
        L.launch(embed_op(self.dtype, cp.img_feat.ptr, cp.n_img * D, out, norm, n, D), self.stream)
        return out

    def _caption_chunks(self, src, n_all, chunk, R, max_new_tokens, beam, fill, prompt=None, scores=False, controls=None, vocab=None,
                        embeds=None, after=None):
        """encode + decode n_all images in chunks of `chunk` on the captioner's stream, each on the plan of its bucket: fill(cp, s, n)
        writes images [s, s + n) into rows [0, n) of that plan's input (`src`: the tensor they come from).  prompt: `prompt_batch`
        of the n_all images (None = the default prompt).  The `_run` result of every chunk, for `_results` (scores: plans that
        also return the token log-probabilities, for `_results_scores`).  controls: non-neutral `GenerationControls` (None = the
        plans without them): every chunk runs on a controls plan, its block uploaded on the stream before the first step.  vocab: a
        checked `CaptionVocabulary` (None = none): every chunk runs on a vocabulary plan, the trie block uploaded the same way.
        after: after(cp, n) is called behind every chunk's last step, on the stream, INSTEAD of the read-back; its results are the parts."""
        n_txt = prompt[2] if prompt else None
        block = controls.pack(self.w.vocab, self.w.forced_bos) if controls else None
        trie = vocab.pack() if vocab else None
        chunk = min(chunk, self.long_plan_rows(max_new_tokens, beam[0] if beam else 1))     # 128 up to T = 227: as before
        if src.is_cuda:                                     # pixels / a screenshot the caller is still producing on its own stream
            self.stream.wait_stream(torch.cuda.current_stream(src.device))
        parts = []
        for s in range(0, n_all, chunk):
            n = min(chunk, n_all - s)
            cp = self.plans(self.bucket(n), R, max_new_tokens, beam=beam, n_txt=n_txt, **({"scores": True} if scores else {}),
                            **({"controls": True} if controls else {}), **({"vocab": True} if vocab else {}))
            with torch.cuda.stream(self.stream):
                cp.reset()
                if controls:
                    cp.set_controls(block)
                if vocab:
                    cp.set_vocabulary(trie)
                fill(cp, s, n)
                if prompt:
                    cp.set_prompt(prompt[0][s:s + n].to(self.device, non_blocking=True), prompt[1][s:s + n].to(self.device, non_blocking=True), n)
                parts.append(self._run(cp, n, max_new_tokens, **({"embeds": embeds} if embeds is not None else {}),
                                       **({"after": after} if after is not None else {})))
        return parts

    def _embed_chunks(self, src, n_all, chunk, R, fill) -> torch.Tensor:
        """f32 [n_all, D] on the device: the embed-only plan of each chunk's bucket on the captioner's stream, chunked as
        `_caption_chunks` chunks; fill(cp, s, n) as there"""
        D = self.w.d_model
        out = torch.empty((n_all, D), dtype=torch.float32, device=self.device)
        if self.device.type == "cuda":                      # `out` comes from the caller's stream, as pixels / a screenshot may
            self.stream.wait_stream(torch.cuda.current_stream(self.device))
            out.record_stream(self.stream)
        for s in range(0, n_all, chunk):
            n = min(chunk, n_all - s)
            cp = self.embed_plans(self.bucket(n), R)
            with torch.cuda.stream(self.stream):
                fill(cp, s, n)
                (cp.encode_plan.replay if self.use_graph else cp.encode_plan.run)(self.stream)
                out[s:s + n].copy_(cp.emb[:n], non_blocking=True)
        if self.device.type == "cuda":
            torch.cuda.current_stream(self.device).wait_stream(self.stream)     # the caller reads `out` on its own stream
        return out

    @torch.inference_mode()
    def embed(self, pixel_values) -> torch.Tensor:
        """Visual embeddings of images: f32 [n, d_model] on the device, unit length.  pixel_values [n, 3, R, R] as `generate` takes
        them.  A row is Florence-2's own global descriptor of the image — row 0 of the image features, the spatial-average token
        behind image_projection and image_proj_norm (transformers' get_image_features(...).pooler_output[:, 0]) — L2-normalised by
        OMNI_OP_VISUAL_MATCH mode 0.  It is a pure function of the pixels: nothing is cached.  It runs the DaViT tower and the
        projector only (the embed-only plan of `embed_plans`: no encoder, no cross-K/V, no decode step), in chunks of 128 on the
        bucket ladder exactly as `generate` chunks."""
        with self._lock:
            Bn, _, R, R2 = pixel_values.shape
            assert R == R2

            def fill(cp, s, n):
                cp.x_in.t[:n, :, :, :3] = pixel_values[s:s + n].to(self.device).permute(0, 2, 3, 1).to(cp.x_in.t.dtype)
            return self._embed_chunks(pixel_values, Bn, 128, R, fill)

    @torch.inference_mode()
    def embed_crops(self, image_u8: torch.Tensor, boxes_px: List[List[int]], batch_size=128) -> torch.Tensor:
        """`embed` through the device crop path of `caption_crops`: the rectangles `boxes_px` of the HWC uint8 frame on the device
        are cut, resized and normalised there.  f32 [len(boxes_px), d_model] on the device."""
        batch_size = max(1, min(int(batch_size), 128))

        def fill(cp, s, n):
            rects = torch.tensor(boxes_px[s:s + n], dtype=torch.int32).to(self.device, non_blocking=True)
            self.launch_crops(cp, 0, n, image_u8, rects, *self.crop_scratch(n, cp.R), self.stream)
        with self._lock:
            return self._embed_chunks(image_u8, len(boxes_px), batch_size, self.resolution, fill)

    @torch.inference_mode()
    def match(self, queries: torch.Tensor, gallery: torch.Tensor, top_k=1):
        """The best `top_k` gallery rows of every query by cosine similarity: (idx i64 [m, top_k], score f32 [m, top_k]) on the
        device.  queries f32 [.., D] and gallery f32 [.., D] are unit vectors on the device (what `embed` returns); the score is
        their f32 dot product, whose bits for a pair do not depend on what else is in the call.  Descending score, the lower
        gallery index first among equals; behind min(top_k, n) positions hold -1 and -inf.  Two launches of OMNI_OP_VISUAL_MATCH
        (per-slice top-k, merge).  ValueError before anything reaches the device: top_k no int in 1..8, mismatching D, an empty side,
        D no multiple of 4 or above 4096, more than 4096 queries or 65536 gallery rows."""
        check_match_args(queries, gallery, top_k)
        with self._lock:
            return match_topk(queries, gallery, top_k, self.device)

    def _results(self, parts, beam, nrs=1):
        """(sequences, sequences_scores) of the per-chunk `_run` results: beam search as `_beam_outputs`; greedy decoding (scores
        None): every chunk trimmed where hf stops (`_finish_ids`), then padded to the longest"""
        if beam:
            return self._beam_outputs(parts, nrs)
        parts = [self._finish_ids(p) for p in parts]
        T = max(p.shape[1] for p in parts)
        return torch.cat([torch.nn.functional.pad(p, (0, T - p.shape[1]), value=self.w.pad) for p in parts]), None

    def _results_scores(self, parts):
        """(sequences, token_logprobs [B, T - 1]) of the per-chunk (ids, logp) `_run` results of scores plans: trimmed and padded like
        `_results`; the log-probabilities of padding are 0"""
        ids = [self._finish_ids(p[0]) for p in parts]
        T = max(p.shape[1] for p in ids)
        seq = torch.cat([torch.nn.functional.pad(p, (0, T - p.shape[1]), value=self.w.pad) for p in ids])
        logp = torch.cat([torch.nn.functional.pad(p[1][:, 1:i.shape[1]], (0, T - i.shape[1])) for p, i in zip(parts, ids)])
        return seq, logp.float().contiguous()

    def _beam_outputs(self, parts, nrs):
        """hf's output of _beam_search (generation/utils.py:3508-3523) from per-chunk (ids [n,k,T], scores [n,k], lengths [n,k]): the
        best `nrs` hypotheses per image, trimmed to 1 + the longest generated length among the returned ones."""
        ids = torch.cat([p[0][:, :nrs] for p in parts]).flatten(0, 1)
        scores = torch.cat([p[1][:, :nrs] for p in parts]).flatten(0, 1)
        lens = torch.cat([p[2][:, :nrs] for p in parts]).flatten(0, 1)
        T = 1 + int(lens.max()) if lens.numel() else 1
        return ids[:, :T].contiguous(), scores

    @torch.inference_mode()
    def caption_crops(self, image_u8: torch.Tensor, boxes_px: List[List[int]], max_new_tokens=20, batch_size=128, num_beams=None,
                      prompt_ids=None, return_scores=None, controls=None, vocabulary=None, return_embeddings=False):
        """Fused fast path: crops are cut, resized (cv2-bilinear 64x64, then Pillow-bicubic to R on the
        768 path) and normalised on device from the HBM-resident screenshot (ref:util/utils.py:97-123).
        num_beams: None = `self.num_beams` (default 1, greedy); k > 1 = beam search, the best hypothesis per crop (what
        generate(num_beams=k) returns for the same pixels).
        prompt_ids: one list of token ids (bos ... eos) for all crops, None = the default PROMPT_IDS; see `prompt_batch`.
        return_scores: None = `self.token_scores` (default False); True returns (ids, token_logprobs) — f32 [n, ids.shape[1] - 1],
        aligned with ids[:, 1:], see `generate(output_scores=True)` and `caption_confidence`; greedy decoding only.
        controls: a `GenerationControls` or a dict of its keys (repetition_penalty, no_repeat_ngram_size, min_new_tokens,
        suppress_tokens, begin_suppress_tokens, bad_words_ids), see `generate`; None or neutral = the call as it was.
        vocabulary: a `CaptionVocabulary` or a list of labels as id lists, see `generate`: every row is one of the labels
        (`CaptionVocabulary.label_index` names it); greedy decoding without controls only; None = the call as it was.
        return_embeddings: True appends the crops' visual embeddings (f32 [n, d_model] on the device, what `embed_crops` returns
        for the same boxes) to the result: (ids, embeddings), or (ids, token_logprobs, embeddings) with scores.  They are read off
        the caption plan's own image features by one eager OMNI_OP_VISUAL_MATCH launch behind each chunk's encode plan — one
        encode, not two; the captured graphs are what they were.  Any decoding mode (img_feat does not depend on it).  False
        (default) = the call as it was."""
        if not isinstance(return_embeddings, bool):
            raise ValueError(f"return_embeddings must be a bool, got {return_embeddings!r}")
        embeds = [] if return_embeddings else None
        beam = self.beam_config(num_beams)
        scores = self.token_scores if return_scores is None else return_scores
        if not isinstance(scores, bool):
            raise ValueError(f"return_scores must be a bool or None, got {scores!r}")
        if scores and beam:
            raise ValueError("token scores are a greedy-decoding output (num_beams=1); beam search has none")
        self.check_max_new(max_new_tokens, beam)
        controls = self.generation_controls(controls, max_new_tokens, beam)
        vocab = self.caption_vocabulary(vocabulary, max_new_tokens, beam, controls)
        prompt = self.prompt_batch([list(prompt_ids)] * len(boxes_px), self.resolution) if prompt_ids is not None and len(boxes_px) else None
        batch_size = max(1, min(int(batch_size), 128))      # plan capacity: buckets stop at 128 crops (the reference's default batch)

        def fill(cp, s, n):
            rects = torch.tensor(boxes_px[s:s + n], dtype=torch.int32).to(self.device, non_blocking=True)
            self.launch_crops(cp, 0, n, image_u8, rects, *self.crop_scratch(n, cp.R), self.stream)
        with self._lock:
            parts = self._caption_chunks(image_u8, len(boxes_px), batch_size, self.resolution, max_new_tokens, beam, fill, prompt, scores, controls, vocab,
                                         **({"embeds": embeds} if return_embeddings else {}))
        emb = ()
        if return_embeddings:
            emb = (torch.cat(embeds) if embeds else torch.zeros((0, self.w.d_model), dtype=torch.float32, device=self.device),)
        if not parts:
            ids = torch.zeros((0, 1), dtype=torch.long)
            out = (ids, torch.zeros((0, 0), dtype=torch.float32)) if scores else (ids,)
        elif scores:
            out = self._results_scores(parts)
        else:
            out = (self._results(parts, beam)[0],)
        return out[0] if len(out + emb) == 1 else tuple(out) + emb

    # ---- region OCR over native-resolution tiles (OMNI_OP_REGION_OCR)
    def launch_tiles(self, cp, n, image_u8, origins, stream):
        """one OMNI_OP_REGION_OCR mode-0 launch on `stream`: the n windows of cp.R x cp.R pixels at `origins` (int32 [n, 2] x y on the
        device) of one HWC uint8 frame, normalised into rows [0, n) of cp.x_in; pixels outside the frame are white"""
        lut, _ = self._crop_tables(64)
        H, W = image_u8.shape[:2]
        L.launch(tile_cut_op(self.dtype, image_u8.data_ptr(), origins.data_ptr(), cp.x_in.ptr, lut.data_ptr(), n, H, W, cp.R, cp.x_in.ld), stream)

    @torch.inference_mode()
    def read_regions(self, image_u8: torch.Tensor, max_new_tokens=1024, overlap=128, prompt_ids=None, class_table=None, controls=None):
        """Read the text of a screenshot with its places: Florence-2's <OCR_WITH_REGION> task over tiles of the captioner's own
        resolution R, cut from the HWC uint8 frame on the device WITHOUT resizing (a whole frame squeezed to R x R is unreadable).
        Tiles: `ScreenParser.tile_origins(W, H, R, R, overlap)`, row-major; they are the rows of the chunked greedy decode
        `describe_image` runs (scores plans, `long_plan_rows` per chunk, the early-exit poll), filled by OMNI_OP_REGION_OCR mode 0;
        mode 1 parses every chunk's ids and log-probabilities on the device behind its last step.  One read-back at the end.
        prompt_ids: the task's prompt (bos ... eos), `FlorenceProcessor.prompt_ids("<OCR_WITH_REGION>")`; class_table: the u16
        per-token class table, `FlorenceProcessor.loc_class_table()`; controls: as in `caption_crops`.
        Returns an object with `origins` [(x, y)] per tile, `records` i32 [tiles, M, 16], `sums` f32 [tiles, M], `rows` i32 [tiles, 4]
        `ids` i64 [tiles, T] and `logp` f32 [tiles, T - 1] aligned with ids[:, 1:] (for rows re-parsed on the host)
        (T = max_new_tokens + 1, M = (T - 1) // 9) — the op's outputs as include/omni_amd.h describes them:
        a region's content as a column range of `ids`, its quad in frame pixels, its token count and log-probability sum, and whether
        its own tile keeps it (`ocr_cells`); per tile the regions found and kept and the flags (1: a token the device does not parse
        — re-parse the row from text; 2: cut off at max_new_tokens).
        ValueError before anything reaches the device: no prompt or class table, overlap outside 0 <= overlap < R, max_new_tokens
        outside `check_max_new`, a frame that is not HWC uint8, bad controls."""
        R = int(self.resolution)
        if prompt_ids is None or class_table is None:
            raise ValueError("read_regions needs prompt_ids (the <OCR_WITH_REGION> prompt) and class_table (FlorenceProcessor.loc_class_table())")
        table = check_class_table(class_table)
        if isinstance(overlap, bool) or not isinstance(overlap, int) or not 0 <= overlap < R:
            raise ValueError(f"overlap must be an integer in 0..{R - 1} (tiles are {R} x {R}), got {overlap!r}")
        self.check_max_new(max_new_tokens)
        controls = self.generation_controls(controls, max_new_tokens, None)
        if not isinstance(image_u8, torch.Tensor) or image_u8.dtype != torch.uint8 or image_u8.dim() != 3 or image_u8.shape[2] != 3 \
                or image_u8.shape[0] < 1 or image_u8.shape[1] < 1:
            raise ValueError("image_u8 must be a uint8 tensor [H, W, 3]")
        from .pipeline import ScreenParser
        H, W = int(image_u8.shape[0]), int(image_u8.shape[1])
        origins = ScreenParser.tile_origins(W, H, R, R, overlap)[0]
        n_all, T = len(origins), max_new_tokens + 1
        M = ocr_slots(T)
        prompt = self.prompt_batch([list(prompt_ids)] * n_all, R)
        dev = self.device
        image_u8 = image_u8.to(dev).contiguous()
        with self._lock:
            if image_u8.is_cuda:               # a screenshot the caller is still producing on its own stream
                self.stream.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(self.stream):
                org =torch.tensor(origins, dtype=torch.int32).to(dev, non_blocking=True)
                cells = torch.tensor(ocr_cells(origins, R), dtype=torch.int32).to(dev, non_blocking=True)
                tab = table.to(dev, non_blocking=True)
                rec = torch.zeros((n_all, max(M, 1), 16), dtype=torch.int32, device=dev)
                sums = torch.zeros((n_all, max(M, 1)), dtype=torch.float32, device=dev)
                rows = torch.zeros((n_all, 4), dtype=torch.int32, device=dev)
                ids = torch.full((n_all, T), int(self.w.pad), dtype=torch.int32, device=dev)     # columns no step reached: pad
                logp = torch.zeros((n_all, T), dtype=torch.float32, device=dev)
            at = [0]

            def fill(cp, s, n):
                at[0] = s
                self.launch_tiles(cp, n, image_u8, org[s:s + n], self.stream)

            def after(cp, n):
                s = at[0]
                L.launch(region_parse_op(cp.ids.data_ptr(), tab.data_ptr(), cp.logp.data_ptr() + 4, cells[s:s + n].data_ptr(),
                                         rec[s:s + n].data_ptr(), sums[s:s + n].data_ptr(), rows[s:s + n].data_ptr(), n, T, tab.numel(), R,
                                         int(self.w.eos), ld_ids=T, ld_logp=T), self.stream)
                done = self.last_steps + 1             # the early exit leaves the columns behind it as `reset` left them
                ids[s:s + n, :done].copy_(cp.ids[:n, :done], non_blocking=True)
                logp[s:s + n, :done].copy_(cp.logp[:n, :done], non_blocking=True)

            self._caption_chunks(image_u8, n_all, 128, R, max_new_tokens, None, fill, prompt, True, controls, after=after)
            with torch.cuda.stream(self.stream):
                out = SimpleNamespace(origins=origins, records=rec[:, :M].cpu(), sums=sums[:, :M].cpu(), rows=rows.cpu(), ids=ids.cpu().long(),
                                      logp=logp[:, 1:].cpu())
        return out

    # ---- box answers and region prompts over tiles (OMNI_OP_REGION_OCR modes 0 and 3)
    def _check_frame_rows(self, image_u8, prompts, max_new_tokens, controls):
        """the argument checks `decode_tiles` and `locate_regions` share -> (prompt rows as int lists, checked controls)"""
        rows = [[int(t) for t in (r.tolist() if isinstance(r, torch.Tensor) else r)] for r in (prompts if prompts is not None else [])]
        if not rows:
            raise ValueError("no prompts: at least one prompt row (bos ... eos) is needed")
        for r in rows:
            text_capacity(len(r))
        self.check_max_new(max_new_tokens)
        controls = self.generation_controls(controls, max_new_tokens, None)
        if not isinstance(image_u8, torch.Tensor) or image_u8.dtype != torch.uint8 or image_u8.dim() != 3 or image_u8.shape[2] != 3 \
                or image_u8.shape[0] < 1 or image_u8.shape[1] < 1:
            raise ValueError("image_u8 must be a uint8 tensor [H, W, 3]")
        return rows, controls

    @torch.inference_mode()
    def decode_tiles(self, image_u8: torch.Tensor, origins, prompts, max_new_tokens, controls=None, parse=None, fetch=None):
        """Greedy answers for windows of a frame, each under its own prompt: one row per (origin, prompt) pair.  The window of
        R x R pixels (R = the captioner's resolution) at origin (x, y) is cut from the HWC uint8 frame on the device, unscaled, white
        outside the frame (OMNI_OP_REGION_OCR mode 0); the rows run the chunked greedy decode of `read_regions` (scores plans,
        `long_plan_rows` rows per chunk, the early-exit poll) with per-row prompts.  prompts: token rows (bos ... eos), as many as
        origins.  One read-back at the end.  Returns an object with `ids` i64 [rows, T] and `logp` f32 [rows, T - 1] aligned with
        ids[:, 1:] (T = max_new_tokens + 1; columns no step reached hold the pad token and 0).
        parse: parse(s, n, cp) is called on the captioner's stream behind the last step of the chunk that holds rows [s, s + n),
        cp.ids / cp.logp being that chunk's [.., T] buffers — where `locate_regions` launches its parser; fetch: {name: device tensor}
        read back with the ids, as attributes of the result.
        ValueError before anything reaches the device: no prompt, a prompt of more than 64 tokens or with an id outside the token
        table, origins and prompts of different lengths, max_new_tokens outside `check_max_new`, a frame that is not HWC uint8, bad
        controls."""
        R = int(self.resolution)
        rows, controls = self._check_frame_rows(image_u8, prompts, max_new_tokens, controls)
        origins = [(int(x), int(y)) for x, y in origins]
        if len(origins) != len(rows):
            raise ValueError(f"{len(origins)} origins for {len(rows)} prompts: one prompt per origin is needed")
        if any(abs(v) > 2 ** 30 for o in origins for v in o):
            raise ValueError("origins must lie within +-2^30")
        n_all, T = len(rows), max_new_tokens + 1
        prompt = self.prompt_batch(rows, R)
        dev = self.device
        image_u8 = image_u8.to(dev).contiguous()
        with self._lock:
            if image_u8.is_cuda:               # a screenshot the caller is still producing on its own stream
                self.stream.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(self.stream):
                org = torch.tensor(origins, dtype=torch.int32).to(dev, non_blocking=True)
                ids = torch.full((n_all, T), int(self.w.pad), dtype=torch.int32, device=dev)     # columns no step reached: pad
                logp = torch.zeros((n_all, T), dtype=torch.float32, device=dev)
            at = [0]

            def fill(cp, s, n):
                at[0] = s
                self.launch_tiles(cp, n, image_u8, org[s:s + n], self.stream)

            def after(cp, n):
                s = at[0]
                if parse is not None:
                    parse(s, n, cp)
                done = self.last_steps + 1             # the early exit leaves the columns behind it as `reset` left them
                ids[s:s + n, :done].copy_(cp.ids[:n, :done], non_blocking=True)
                logp[s:s + n, :done].copy_(cp.logp[:n, :done], non_blocking=True)

            self._caption_chunks(image_u8, n_all, 128, R, max_new_tokens, None, fill, prompt, True, controls, after=after)
            with torch.cuda.stream(self.stream):
                out = SimpleNamespace(ids=ids.cpu().long(), logp=logp[:, 1:].cpu(), **{k: t.cpu() for k, t in (fetch or {}).items()})
        return out

    @torch.inference_mode()
    def locate_regions(self, image_u8: torch.Tensor, prompts, class_table, grammar, max_new_tokens=1024, overlap=128, controls=None):
        """Box answers over the tiles of a screenshot: every prompt of `prompts` (token rows bos ... eos of a Florence-2 task that
        answers "phrase <loc>x4 ...": <OD>, <DENSE_REGION_CAPTION>, <OPEN_VOCABULARY_DETECTION>, <CAPTION_TO_PHRASE_GROUNDING>, grammar
        0; or boxes alone: <REGION_PROPOSAL>, grammar 1) is put to every tile of `ScreenParser.tile_origins(W, H, R, R, overlap)`.
        Rows = prompts x tiles, prompt-major; they are `decode_tiles` rows, and OMNI_OP_REGION_OCR mode 3 parses every chunk's ids and
        log-probabilities on the device behind its last step.  One read-back at the end.  class_table: as in `read_regions`.
        Returns an object with per row `origins` [(x, y)], `prompt_index` and `tile_index`, `records` i32 [rows, M, 16], `sums` f32
        [rows, M, 2], `rows` i32 [rows, 4], `ids` i64 [rows, T] and `logp` f32 [rows, T - 1] (T = max_new_tokens + 1, M = (T - 1) // 4)
        — the op's outputs as include/omni_amd.h describes them: per box its corners in frame pixels, the columns of its phrase, the
        phrase's ordinal and `lead`, whether its own tile keeps it (`ocr_cells`), and the log-probability sums of the phrase and of
        the box's four location tokens; per row the boxes found and kept, the flags (1: re-parse the row from text, 2: cut off at
        max_new_tokens) and the phrases found.
        ValueError before anything reaches the device: as `decode_tiles` and `read_regions`, and a grammar outside 0..1."""
        R = int(self.resolution)
        if class_table is None:
            raise ValueError("locate_regions needs class_table (FlorenceProcessor.loc_class_table())")
        table = check_class_table(class_table)
        if isinstance(grammar, bool) or grammar not in (0, 1):
            raise ValueError(f"grammar must be 0 (phrases with boxes) or 1 (boxes only), got {grammar!r}")
        if isinstance(overlap, bool) or not isinstance(overlap, int) or not 0 <= overlap < R:
            raise ValueError(f"overlap must be an integer in 0..{R - 1} (tiles are {R} x {R}), got {overlap!r}")
        prompts, _ = self._check_frame_rows(image_u8, prompts, max_new_tokens, controls)
        self.prompt_batch(prompts, R)                      # (an id outside the token table)
        from .pipeline import ScreenParser
        H, W = int(image_u8.shape[0]), int(image_u8.shape[1])
        tiles = ScreenParser.tile_origins(W, H, R, R, overlap)[0]
        origins = list(tiles) * len(prompts)
        prompt_index = [p for p in range(len(prompts)) for _ in tiles]
        tile_index = list(range(len(tiles))) * len(prompts)
        n_all, T = len(origins), max_new_tokens + 1
        M = box_slots(T)
        dev = self.device
        with self._lock:
            with torch.cuda.stream(self.stream):
                cells = torch.tensor(ocr_cells(origins, R), dtype=torch.int32).to(dev, non_blocking=True)
                tab = table.to(dev, non_blocking=True)
                rec = torch.zeros((n_all, max(M, 1), 16), dtype=torch.int32, device=dev)
                sums = torch.zeros((n_all, max(M, 1), 2), dtype=torch.float32, device=dev)
                rows = torch.zeros((n_all, 4), dtype=torch.int32, device=dev)

            def parse(s, n, cp):
                L.launch(box_parse_op(cp.ids.data_ptr(), tab.data_ptr(), cp.logp.data_ptr() + 4, cells[s:s + n].data_ptr(),
                                      rec[s:s + n].data_ptr(), sums[s:s + n].data_ptr(), rows[s:s + n].data_ptr(), n, T, tab.numel(), R,
                                      int(self.w.eos), int(grammar), ld_ids=T, ld_logp=T), self.stream)

            out = self.decode_tiles(image_u8, origins, [prompts[p] for p in prompt_index], max_new_tokens, controls, parse=parse,
                                    fetch={"records": rec[:, :M], "sums": sums[:, :M], "rows": rows})
        out.origins, out.prompt_index, out.tile_index = origins, prompt_index, tile_index
        return out

    # ---- polygon answers and bit masks over tiles (OMNI_OP_REGION_OCR modes 0, 5 and 6)
    @torch.inference_mode()
    def segment_regions(self, image_u8: torch.Tensor, origins, prompts, class_table, max_new_tokens=256, instances=4, masks=True,
                        controls=None, cells=None):
        """Polygon answers and their masks for windows of a screenshot: `decode_tiles` rows (origin, prompt) whose prompts are those of
        <REFERRING_EXPRESSION_SEGMENTATION> or <REGION_TO_SEGMENTATION> (`FlorenceProcessor.segment_prompt_ids`).  Behind the last step
        of every chunk OMNI_OP_REGION_OCR mode 5 parses the chunk's ids and log-probabilities into polygons on the device and, with
        `masks`, mode 6 rasters the first `instances` instances of every row into tile-local bit masks from mode 5's outputs where they
        lie.  One read-back at the end.  class_table: `FlorenceProcessor.poly_class_table()`.  cells: per row [origin x, origin y, lo x,
        hi x, lo y, hi y], the cell whose instances the row keeps (as `ocr_cells` writes them; the origins must be the row's); None =
        `ocr_cells(origins, R)`, the grid the given origins span — right when the rows are every tile of a frame's grid, while rows put
        to single tiles on purpose want cells without ends (-2^31, OCR_INF).
        Returns `decode_tiles`' object with `origins`, `vertices` i32 [rows, V, 2], `records` i32 [rows, P, 16], `sums` f32 [rows, P],
        `rows` i32 [rows, 4] and, with `masks`, `masks` i32 [rows, instances, R, (R + 31) // 32] (the bits of u32 words) and `counts` i32
        [rows, instances, R] (T = max_new_tokens + 1; P, V = poly_slots(T)) — the op's outputs as include/omni_amd.h describes them.
        ValueError before anything reaches the device: `decode_tiles`' own, no class table, max_new_tokens below 2, `instances` outside
        1..64, cells that are not one row of six 32-bit integers per origin starting with that origin."""
        R = int(self.resolution)
        if class_table is None:
            raise ValueError("segment_regions needs class_table (FlorenceProcessor.poly_class_table())")
        table = check_class_table(class_table)
        if isinstance(instances, bool) or not isinstance(instances, int) or not 1 <= instances <= 64:
            raise ValueError(f"instances must be an integer in 1..64 (mask slots per row), got {instances!r}")
        prompts, _ = self._check_frame_rows(image_u8, prompts, max_new_tokens, controls)
        if max_new_tokens < 2:
            raise ValueError("max_new_tokens must be at least 2: a polygon answer has no room in one token")
        self.prompt_batch(prompts, R)                      # (an id outside the token table)
        origins = [(int(x), int(y)) for x, y in origins]
        if len(origins) != len(prompts):
            raise ValueError(f"{len(origins)} origins for {len(prompts)} prompts: one prompt per origin is needed")
        if any(abs(v) > 2 ** 30 for o in origins for v in o):
            raise ValueError("origins must lie within +-2^30")
        cell_rows = ocr_cells(origins, R) if cells is None else [[int(v) for v in c] for c in cells]
        if len(cell_rows) != len(origins) or any(len(c) != 6 or (c[0], c[1]) != o or not all(-2 ** 31 <= v <= OCR_INF for v in c)
                                                 for c, o in zip(cell_rows, origins)):
            raise ValueError("cells must hold one row [origin x, origin y, lo x, hi x, lo y, hi y] of 32-bit integers per origin")
        H, W = int(image_u8.shape[0]), int(image_u8.shape[1])
        n_all, T, I, WR = len(origins), max_new_tokens + 1, int(instances), (R + 31) // 32
        P, V = poly_slots(T)
        dev = self.device
        with self._lock:
            with torch.cuda.stream(self.stream):
                cells = torch.tensor(cell_rows, dtype=torch.int32).to(dev, non_blocking=True)
                tab = table.to(dev, non_blocking=True)
                verts = torch.zeros((n_all, V, 2), dtype=torch.int32, device=dev)
                rec = torch.zeros((n_all, P, 16), dtype=torch.int32, device=dev)
                sums = torch.zeros((n_all, P), dtype=torch.float32, device=dev)
                rows = torch.zeros((n_all, 4), dtype=torch.int32, device=dev)
                fetch = {"vertices": verts, "records": rec, "sums": sums, "rows": rows}
                if masks:
                    fetch["masks"] = torch.zeros((n_all, I, R, WR), dtype=torch.int32, device=dev)
                    fetch["counts"] = torch.zeros((n_all, I, R), dtype=torch.int32, device=dev)

            def parse(s, n, cp):
                L.launch(poly_parse_op(cp.ids.data_ptr(), tab.data_ptr(), cp.logp.data_ptr() + 4, cells[s:s + n].data_ptr(), verts[s:s + n].data_ptr(),
                                       rec[s:s + n].data_ptr(), sums[s:s + n].data_ptr(), rows[s:s + n].data_ptr(), n, T, tab.numel(), R,
                                       int(self.w.eos), ld_ids=T, ld_logp=T), self.stream)
                if masks:
                    L.launch(poly_mask_op(rec[s:s + n].data_ptr(), rows[s:s + n].data_ptr(), verts[s:s + n].data_ptr(), cells[s:s + n].data_ptr(),
                                          fetch["masks"][s:s + n].data_ptr(), fetch["counts"][s:s + n].data_ptr(), n, T, I, H, W, R), self.stream)

            out = self.decode_tiles(image_u8, origins, prompts, max_new_tokens, controls, parse=parse, fetch=fetch)
        out.origins = origins
        return out

    # ---- teacher-forced scoring of given texts (OMNI_OP_GREEDY_STEP p5)
    def _check_labels(self, labels, n):
        """`score`'s labels -> (per image a list of M token lists, M, shared).  ValueError: no label, an empty label, more than
        LABEL_CAPACITIES[-1] tokens, an id outside the vocabulary, a per-image list of another length than the images."""
        tolist = lambda x: x.tolist() if isinstance(x, torch.Tensor) else list(x)
        labels = [tolist(r) for r in tolist(labels)] if labels is not None else []
        if not labels:
            raise ValueError("no labels: at least one candidate text is needed")
        shared = not (labels[0] and isinstance(labels[0][0], (list, tuple, torch.Tensor)))      # a flat list of ids: one label
        per = [labels] if shared else [[tolist(r) for r in rows] for rows in labels]
        if not shared and len(per) != n:
            raise ValueError(f"{len(per)} label lists for {n} images")
        vocab = min(self.w.vocab, self.w.sd["model.language_model.shared.weight"].shape[0])     # scored by the lm_head, embedded from the table
        out = []
        for rows in per:
            rows = [[int(t) for t in r] for r in rows]
            if not rows:
                raise ValueError("no labels: at least one candidate text is needed")
            if len(rows) != len(per[0]):
                raise ValueError("every image needs the same number of labels")
            for r in rows:
                if not r:
                    raise ValueError("an empty label: at least one token is needed")
                if len(r) > LABEL_CAPACITIES[-1]:
                    raise ValueError(f"a label of {len(r)} tokens exceeds the limit of {LABEL_CAPACITIES[-1]}")
                bad = [t for t in r if not 0 <= t < vocab]
                if bad:
                    raise ValueError(f"label token id {bad[0]} is outside the vocabulary (0..{vocab - 1})")
            out.append(rows)
        return out, len(out[0]), shared

    def _score_chunks(self, src, n_all, chunk, R, per, M, shared, fill, prompt=None):
        """encode n_all images in chunks of `chunk` and score their M labels: per chunk ONE encode, then one pass of the step plan per
        FORCE_ROWS[-1] labels (reset of the step state, new ids / lengths, max(length) steps: the host knows them, nothing is polled)."""
        Lmax = max(len(r) for rows in per for r in rows)
        cap_l = next(c for c in LABEL_CAPACITIES if Lmax <= c)
        Mp = next(m for m in FORCE_ROWS if min(M, FORCE_ROWS[-1]) <= m)
        T = cap_l + 1
        n_txt = prompt[2] if prompt else None
        if src.is_cuda:
            self.stream.wait_stream(torch.cuda.current_stream(src.device))
        run = (lambda p: p.replay(self.stream)) if self.use_graph else (lambda p: p.run(self.stream))
        stats = self.score_stats = {"encodes": 0, "passes": 0, "steps": 0}
        logp = torch.zeros((n_all, M, Lmax), dtype=torch.float32)
        top1 = torch.zeros((n_all, M, Lmax), dtype=torch.long)
        for s in range(0, n_all, chunk):
            n = min(chunk, n_all - s)
            cp = self.plans(self.bucket(n), R, cap_l, n_txt=n_txt, force=Mp)
            snaps = []
            with torch.cuda.stream(self.stream):
                fill(cp, s, n)
                if prompt:
                    cp.set_prompt(prompt[0][s:s + n].to(self.device, non_blocking=True), prompt[1][s:s + n].to(self.device, non_blocking=True), n)
                run(cp.encode_plan)
                stats["encodes"] += 1
                for m0 in range(0, M, Mp):
                    m1 = min(M, m0 + Mp)
                    ids = torch.full((cp.B, Mp, T), int(self.w.pad), dtype=torch.int32)
                    ids[:, :, 0] = int(self.w.start)
                    tlen = torch.zeros((cp.B, Mp), dtype=torch.int32)
                    for b in range(n):
                        for j, r in enumerate((per[0] if shared else per[s + b])[m0:m1]):
                            ids[b, j, 1:1 + len(r)] = torch.tensor(r, dtype=torch.int32)
                            tlen[b, j] = len(r)
                    cp.reset()
                    cp.set_targets(ids.view(-1, T), tlen.view(-1))
                    steps = int(tlen.max())
                    for _ in range(steps):
                        run(cp.step_plan)
                    stats["passes"] += 1
                    stats["steps"] += steps
                    snaps.append((m0, m1, cp.logp.view(cp.B, Mp, T)[:n, :m1 - m0, 1:1 + Lmax].clone(),
                                  cp.top1.view(cp.B, Mp, T)[:n, :m1 - m0, 1:1 + Lmax].clone()))
                for m0, m1, lp, t1 in snaps:             # read back behind the last pass, on the stream that wrote them (synchronises it)
                    logp[s:s + n, m0:m1] = lp.cpu()
                    top1[s:s + n, m0:m1] = t1.cpu().long()
        lengths = torch.tensor([[len(r) for r in (per[0] if shared else per[b])] for b in range(n_all)], dtype=torch.long).view(n_all, M)
        return SimpleNamespace(token_logprobs=logp, lengths=lengths, top1=top1)

    @torch.inference_mode()
    def score(self, pixel_values, labels, input_ids=None, attention_mask=None):
        """How likely are given texts, given an image?  The teacher-forced counterpart of `generate`, what transformers computes with
        `model(input_ids, pixel_values, labels=labels)`: per image and label the log-probability of every label token under the RAW
        model distribution log_softmax(logits + final_logits_bias) — no n-gram ban, no forced token (unlike `generate`'s
        token_logprobs, which follow the processed scores and are 0 at forced positions).

        labels: a list of M token lists shared by all images, or one such list per image.  A label is [bos, ..., eos], exactly what
        `FlorenceProcessor.prompt_ids(text)` returns and what transformers calls `labels`; the decoder reads
        shift_tokens_right(labels, pad, decoder_start_token_id).  input_ids / attention_mask: the prompt, as in `generate`.
        Returns an object with `token_logprobs` f32 [n, M, Lmax] (aligned with the labels, 0 behind a label's end), `lengths`
        [n, M] and `top1` [n, M, Lmax] (the model's own arg-max at every label position).  See `sequence_score`.
        The M labels of a crop are rows of one decode over ONE encode (up to 8 at a time; more take further passes of the step
        loop over the same encoded crops).  ValueError: see `_check_labels`."""
        with self._lock:
            Bn, _, R, R2 = pixel_values.shape
            assert R == R2
            per, M, shared = self._check_labels(labels, Bn)
            prompt = self._prompt_from_input_ids(input_ids, attention_mask, Bn, R)

            def fill(cp, s, n):
                cp.x_in.t[:n, :, :, :3] = pixel_values[s:s + n].to(self.device).permute(0, 2, 3, 1).to(cp.x_in.t.dtype)
            return self._score_chunks(pixel_values, Bn, 128, R, per, M, shared, fill, prompt)

    @torch.inference_mode()
    def score_crops(self, image_u8: torch.Tensor, boxes_px: List[List[int]], labels, prompt_ids=None, batch_size=128):
        """`score` on the fused path of `caption_crops`: the crops are cut, resized and normalised on the device from the screenshot.
        labels, result: as `score` (n = len(boxes_px)); prompt_ids: one prompt for all crops, None = PROMPT_IDS."""
        per, M, shared = self._check_labels(labels, len(boxes_px))
        prompt = self.prompt_batch([list(prompt_ids)] * len(boxes_px), self.resolution) if prompt_ids is not None and len(boxes_px) else None
        batch_size = max(1, min(int(batch_size), 128))

        def fill(cp, s, n):
            rects = torch.tensor(boxes_px[s:s + n], dtype=torch.int32).to(self.device, non_blocking=True)
            self.launch_crops(cp, 0, n, image_u8, rects, *self.crop_scratch(n, cp.R), self.stream)
        with self._lock:
            return self._score_chunks(image_u8, len(boxes_px), batch_size, self.resolution, per, M, shared, fill, prompt)

    # ---- device crop pre-processing (OMNI_OP_CROP_RESIZE), shared by caption_crops and ScreenParser
    def _crop_tables(self, R):
        """(1/255 LUT of the u8 -> f32 conversion, (bicubic 64 -> R bounds, weights, taps) or (None, None, 0) at R = 64), built on first use"""
        if self._lut is None:
            self._lut = torch.from_numpy((np.arange(256).astype(np.float64) * (1 / 255)).astype(np.float32)).to(self.device)
        if R != 64 and R not in self._bic:
            b, k = L.resample_coeffs(64, R, 1)
            self._bic[R] = (torch.from_numpy(b).to(self.device), torch.from_numpy(k).to(self.device), k.shape[1])
        return self._lut, self._bic.get(R, (None, None, 0))

    def crop_scratch(self, n, R):
        """device scratch of the crop op for n crops at resolution R: (64x64 crops, 64-row intermediate of the resize to R or None)"""
        c64 = torch.empty((n, 64, 64, 3), dtype=torch.uint8, device=self.device)
        return c64, (torch.empty((n, 64, R, 3), dtype=torch.uint8, device=self.device) if R != 64 else None)

    def launch_crops(self, cp, row0, n, image_u8, rects, c64, tmp, stream):
        """one OMNI_OP_CROP_RESIZE launch on `stream`: the n rectangles `rects` (int32 [n, 4] x0 y0 x1 y1 on the device) of one HWC
        uint8 frame, cut, resized to cp.R and normalised into rows [row0, row0 + n) of cp.x_in.  c64 / tmp: `crop_scratch` of at
        least n crops, not reused by other streams before the launch has run."""
        R, x = cp.R, cp.x_in
        lut, (bb, kk, ks) = self._crop_tables(R)
        H, W = image_u8.shape[:2]
        ptr = lambda t: t.data_ptr() if t is not None else None
        L.launch(L.make_op(L.OP_CROP_RESIZE, self.dtype,
                           p=[image_u8.data_ptr(), rects.data_ptr(), c64.data_ptr(), ptr(tmp), x.ptr + row0 * R * R * x.ld * x.t.element_size(),
                              ptr(bb), ptr(kk), lut.data_ptr()],
                           i={0: n, 1: H, 2: W, 3: R, 4: ks, 13: x.ld},
                           f={0: CLIP_MEAN[0], 1: CLIP_MEAN[1], 2: CLIP_MEAN[2], 3: CLIP_STD[0], 4: CLIP_STD[1], 5: CLIP_STD[2]}), stream)
