"""Host restatement of the LM's q8_0 KV cache (TEST INFRASTRUCTURE ONLY), shared by test_kv_q8_cpu.py / test_kv_q8_gpu.py.

kv_format="q8_0" (rca_lm_set_kv_format, include/rca.h) keeps every cached head row (64 values of K or of V) as two ggml q8_0 blocks.
The quantiser's input is the fp16 row the default cache would hold, and its rule is the q8_1 rule of tests/lm_q8_1_ref.py (reused
here): per block of 32, d = amax / 127, inv = d != 0 ? 1 / d : 0, q = roundf(x * inv), stored scale d16 = fp16 rne of d.  Attention
multiplies fp16_rne((float)d16 * q): `dequant`.  Q8KVRef is the project's oracle (oracle/lm_ref.py, not edited) whose new K / V rows
pass through dequant(quant(fp16(row))) before they join the cache.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import lm_ref  # noqa: E402

import lm_q8_1_ref as q81  # noqa: E402


def quant_rows(rows: np.ndarray):
    """float16 [..., 64 k] -> (q int8 [..., 64 k], d16 float16 [..., 2 k]); the fp16 -> f32 widening is exact"""
    rows = np.asarray(rows)
    assert rows.dtype == np.float16 and rows.shape[-1] % 32 == 0
    return q81.quantize_q8_1(rows.astype(np.float32))


def dequant(q: np.ndarray, d16: np.ndarray) -> np.ndarray:
    """the values attention stages: fp16_rne((float)d16 * q); the f32 product is exact (11 x 7 significant bits)"""
    q, d16 = np.asarray(q), np.asarray(d16)
    assert q.dtype == np.int8 and d16.dtype == np.float16
    prod = q.reshape(*d16.shape, 32).astype(np.float32) * d16.astype(np.float32)[..., None]
    with np.errstate(over="ignore"):
        return prod.astype(np.float16).reshape(q.shape)


def fake_quant(rows: np.ndarray) -> np.ndarray:
    return dequant(*quant_rows(rows))


def ulp_jitter(rows: np.ndarray, rng) -> np.ndarray:
    """fp16 rows with every element moved by -1, 0 or +1 fp16 ulp at random (what device and oracle may differ by before the quantiser)"""
    step = rng.integers(-1, 2, rows.shape)
    up, dn = np.nextafter(rows, np.float16(np.inf)), np.nextafter(rows, np.float16(-np.inf))
    return np.where(step > 0, up, np.where(step < 0, dn, rows)).astype(np.float16)


class Q8KVRef(lm_ref.LMRef):
    """LMRef whose new K / V rows are fake-quantised before they join the cache.  kvq8 = False switches that off: the eval is then
    LMRef's, bit for bit.  jitter = a numpy Generator moves the fp16 rows by up to one ulp at random BEFORE the quantiser (the CPU
    measurement of how far an fp16-ulp disagreement between device and oracle rows can move the logits)."""

    kvq8 = True
    jitter = None

    def _kvq(self, t: torch.Tensor) -> torch.Tensor:
        """t: f32 tensor holding fp16 values [nkv, S, 64]"""
        if not self.kvq8:
            return t
        rows = t.numpy().astype(np.float16)
        if self.jitter is not None:
            rows = ulp_jitter(rows, self.jitter)
        return torch.from_numpy(fake_quant(rows).astype(np.float32))

    def _eval(self, ids, last_only, drop_keys) -> torch.Tensor:
        if drop_keys is not None:
            raise NotImplementedError("Q8KVRef does not mask keys (drop_keys)")
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
            q = (h @ self.w[p + "self_attn.q_proj.weight"].T).view(S, c.n_heads, c.head_dim).transpose(0, 1)
            k = (h @ self.w[p + "self_attn.k_proj.weight"].T).view(S, c.n_kv_heads, c.head_dim).transpose(0, 1)
            v = (h @ self.w[p + "self_attn.v_proj.weight"].T).view(S, c.n_kv_heads, c.head_dim).transpose(0, 1)
            q = q * cos + lm_ref._rotate_half(q) * sin
            k = k * cos + lm_ref._rotate_half(k) * sin
            if self.kv_dtype is not None:
                k, v = k.to(self.kv_dtype).float(), v.to(self.kv_dtype).float()
            k, v = self._kvq(k.contiguous()), self._kvq(v.contiguous())
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
            x = x + o @ self.w[p + "self_attn.o_proj.weight"].T
            h = self._norm(x, self.w[p + "post_attention_layernorm.weight"])
            g = h @ self.w[p + "mlp.gate_proj.weight"].T
            u = h @ self.w[p + "mlp.up_proj.weight"].T
            x = x + (torch.nn.functional.silu(g) * u) @ self.w[p + "mlp.down_proj.weight"].T
        if last_only:
            x = x[-1:]
        x = self._norm(x, self.w["model.norm.weight"])
        self.n_tokens += S
        return x @ self.w["lm_head.weight"].T


# ------------------------------------------------------------------------------------------------------------------ inputs
def edge_rows(rng, n_pos: int, nkv: int, scale: float = 1.0) -> np.ndarray:
    """fp16 rows [n_pos, nkv, 64]: random N(0, scale) rows whose first positions carry, in both blocks of every head, the classes of
    the rule: 0 all zero / 1 amax carried by a negative value / 2 amax = 65504 / 3 a block whose d underflows in fp16 (amax 2^-24 * 3:
    d = 1.4e-9 rounds to fp16 zero) / 4 exact ties: amax = 127 * 2^-4 and values (n + 1/2) * 2^-4 of both signs (t is exactly n + 1/2)
    / 5 a subnormal-scale block (amax 3e-4: d16 subnormal but not zero)"""
    assert n_pos >= 6
    x = (rng.standard_normal((n_pos, nkv, 64)) * scale).astype(np.float16)
    x[0] = 0
    x[1] = (rng.uniform(-0.5, 0.5, (nkv, 64))).astype(np.float16)
    x[1, :, 5] = x[1, :, 37] = np.float16(-0.75)
    x[2] = (rng.standard_normal((nkv, 64)) * 1000).astype(np.float16)
    x[2, :, 3] = np.float16(65504.0)
    x[2, :, 40] = np.float16(-65504.0)
    x[3] = 0
    x[3, :, 1::2] = np.float16(3 * 2.0 ** -24)
    x[3, :, 0::4] = np.float16(-(2.0 ** -24))
    e = 2.0 ** -4
    n = rng.integers(0, 126, (nkv, 64)) + 0.5
    x[4] = (n * e * rng.choice([-1.0, 1.0], (nkv, 64))).astype(np.float16)        # (n + 1/2) / 16 with n < 126: exact in fp16
    x[4, :, 0] = np.float16(127 * e)
    x[4, :, 32] = np.float16(-127 * e)
    x[5] = (rng.standard_normal((nkv, 64)) * 1e-4).astype(np.float16)
    return x
