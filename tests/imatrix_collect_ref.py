"""The importance-matrix collector's references (TEST INFRASTRUCTURE ONLY): oracle.lm_ref.LMRef._eval restated with taps at the five
points a collecting pass sums -- the input of attn_q / attn_k / attn_v (kind 0), of attn_output (1), of ffn_gate / ffn_up (2), of
ffn_down (3), per layer, and the final norm's rows of every position (4, output.weight) -- giving the float64 column sums of the squared
fp32 activations; and the model, ids and distances the collector's CPU and GPU tests share."""
import functools
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import lm_ref  # noqa: E402

# the model and ids of tests/test_imatrix_gpu.py: the smallest shapes that take the 128-token tiles and cross a pass boundary
INIT_STD, SEED, N_CTX, N_LAYERS = 0.05, 5, 1280, 2
PARTS = (165, 1029)
PAIRS = [(l, k) for l in range(N_LAYERS) for k in range(4)] + [(0, 4)]     # kind 4 has one vector (its layer is ignored)


def config():
    from realtime_codec_agent_amd.llm import LMConfig
    return LMConfig(vocab_size=1000, hidden=256, n_layers=N_LAYERS, n_heads=4, n_kv_heads=2, head_dim=64, ffn=512)


def width(cfg, kind):
    return {1: cfg.n_heads * cfg.head_dim, 3: cfg.ffn}.get(kind, cfg.hidden)


@functools.lru_cache(maxsize=None)
def ids():
    out = np.random.default_rng(77).integers(0, 1000, sum(PARTS)).astype(np.int32)
    out.setflags(write=False)
    return out


class TappedLMRef(lm_ref.LMRef):
    """LMRef whose _eval also adds, per tap, sum over the rows of float64(activation)^2 into self.sums[(layer, kind)], counts the
    tokens and keeps the final norm's rows of every eval (float32 [S, H]) in self.final_rows."""

    def __init__(self, cfg, weights, kv_dtype=torch.float16):
        super().__init__(cfg, weights, kv_dtype)
        self.sums = {}
        self.count = 0
        self.final_rows = []

    def _tap(self, layer, kind, t):
        s = t.double().pow(2).sum(0).numpy()
        self.sums[(layer, kind)] = self.sums.get((layer, kind), 0.0) + s

    def _eval(self, ids, last_only, drop_keys):
        assert not last_only and drop_keys is None
        c = self.cfg
        ids = torch.as_tensor(list(ids), dtype=torch.long)
        S = ids.shape[0]
        pos = torch.arange(self.n_tokens, self.n_tokens + S)
        freqs = pos[:, None].float() * self.inv_freq[None, :]
        emb = torch.cat((freqs, freqs), dim=-1)
        cos, sin = emb.cos()[None], emb.sin()[None]
        x = self.w["model.embed_tokens.weight"][ids]
        G = c.n_heads // c.n_kv_heads
        for l in range(c.n_layers):
            p = f"model.layers.{l}."
            h = self._norm(x, self.w[p + "input_layernorm.weight"])
            self._tap(l, 0, h)
            q = (h @ self.w[p + "self_attn.q_proj.weight"].T).view(S, c.n_heads, c.head_dim).transpose(0, 1)
            k = (h @ self.w[p + "self_attn.k_proj.weight"].T).view(S, c.n_kv_heads, c.head_dim).transpose(0, 1)
            v = (h @ self.w[p + "self_attn.v_proj.weight"].T).view(S, c.n_kv_heads, c.head_dim).transpose(0, 1)
            q = q * cos + lm_ref._rotate_half(q) * sin
            k = k * cos + lm_ref._rotate_half(k) * sin
            if self.kv_dtype is not None:
                k, v = k.to(self.kv_dtype).float(), v.to(self.kv_dtype).float()
            if self.k[l] is not None and self.n_tokens > 0:
                k = torch.cat((self.k[l][:, : self.n_tokens], k), dim=1)
                v = torch.cat((self.v[l][:, : self.n_tokens], v), dim=1)
            self.k[l], self.v[l] = k, v
            T = k.shape[1]
            qg = q.reshape(c.n_kv_heads, G * S, c.head_dim)
            att = (qg @ k.transpose(1, 2)) * (c.head_dim ** -0.5)
            mask = torch.arange(T)[None, :] > (self.n_tokens + torch.arange(S))[:, None]
            att = att.view(c.n_kv_heads, G, S, T).masked_fill(mask[None, None], float("-inf")).softmax(-1).view(c.n_kv_heads, G * S, T)
            o = (att @ v).view(c.n_heads, S, c.head_dim).transpose(0, 1).reshape(S, c.n_heads * c.head_dim)
            self._tap(l, 1, o)
            x = x + o @ self.w[p + "self_attn.o_proj.weight"].T
            h = self._norm(x, self.w[p + "post_attention_layernorm.weight"])
            self._tap(l, 2, h)
            g = h @ self.w[p + "mlp.gate_proj.weight"].T
            u = h @ self.w[p + "mlp.up_proj.weight"].T
            a = torch.nn.functional.silu(g) * u
            self._tap(l, 3, a)
            x = x + a @ self.w[p + "mlp.down_proj.weight"].T
        x = self._norm(x, self.w["model.norm.weight"])
        self._tap(0, 4, x)
        self.final_rows.append(x.numpy().astype(np.float32))
        self.n_tokens += S
        self.count += S
        return x @ self.w["lm_head.weight"].T


@functools.lru_cache(maxsize=None)
def restatement():
    """the tapped restatement after the 165 + 1029 ids, appended as two evals: .sums, .count (1194), .final_rows"""
    cfg = config()
    ref = TappedLMRef(cfg, lm_ref.random_weights(cfg, SEED, INIT_STD))
    off = 0
    with torch.no_grad():
        for n in PARTS:
            ref._eval(ids()[off:off + n].tolist(), False, None)
            off += n
    return ref


def rel_l2(a, b):
    """|a - b| / |b|"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def d_min(sums):
    """the smallest relative L2 distance between any two vectors of equal width (either one as the denominator): what a collector
    that had filed a vector under another slot would show at the least; returns (d_min, the pair of keys)"""
    best, where = np.inf, None
    for ka, a in sums.items():
        for kb, b in sums.items():
            if ka != kb and len(a) == len(b):
                d = rel_l2(a, b)
                if d < best:
                    best, where = d, (ka, kb)
    return best, where
