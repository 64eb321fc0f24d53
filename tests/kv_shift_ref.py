"""CPU reference of the context shift (rca_lm_kv_remove / LlamaForAlternatingCodeChannels.kv_remove) on the torch oracle's cache,
shared by tests/test_kv_shift_cpu.py and tests/test_kv_shift_gpu.py (TEST INFRASTRUCTURE ONLY).

LMRef keeps the cache of layer l as ref.k[l] / ref.v[l], [n_kv_heads, T, 64] float32 tensors that hold fp16-rounded values
(kv_dtype=torch.float16) with a key's RoPE pair at elements d and d + 32 (rotate_half convention, oracle/lm_ref.py:43-45,117-118).
kv_remove_ref cuts columns [p0, p1) and rotates the keys of the kept tail by -(p1 - p0) positions: the angle is formed the way
LMRef forms a position's angle (f32 position times f32 inv_freq, oracle/lm_ref.py:106), cos / sin and the rotation are float64,
the result is rounded once to fp16."""
import torch

from agent_fakes import OracleLLM


def kv_remove_ref(ref, p0: int, p1: int) -> None:
    n = ref.n_tokens
    assert 0 <= p0 <= p1 <= n, (p0, p1, n)
    delta = p1 - p0
    ang = (torch.tensor([delta]).float() * ref.inv_freq).double()          # [32]
    c, s = ang.cos(), ang.sin()
    for l in range(ref.cfg.n_layers):
        if ref.k[l] is None:
            continue
        k, v = ref.k[l][:, :n], ref.v[l][:, :n]
        if delta and p1 < n:
            tail = k[:, p1:].double()
            x1, x2 = tail[..., :32], tail[..., 32:]
            rot = torch.cat((x1 * c + x2 * s, x2 * c - x1 * s), dim=-1)
            rot = rot.to(torch.float16).float() if ref.kv_dtype is not None else rot.float()
            k = torch.cat((k[:, :p0], rot), dim=1)
        else:
            k = torch.cat((k[:, :p0], k[:, p1:]), dim=1)
        ref.k[l], ref.v[l] = k, torch.cat((v[:, :p0], v[:, p1:]), dim=1)
    ref.n_tokens = n - delta


class ShiftOracleLLM(OracleLLM):
    """OracleLLM with the kv_remove of the HIP LM object, on the oracle's cache."""

    def kv_remove(self, p0, p1):
        kv_remove_ref(self.ref, int(p0), int(p1))
