"""The LM shape sweep shared by tests/test_lm_shapes_cpu.py (is the table what it says it is?) and tests/test_lm_shapes_gpu.py
(does the HIP library compute these shapes right?).

rca_lm_create accepts query group sizes 1 / 2 / 4, any hidden / ffn that is a multiple of 8 (ffn above 2048 in steps of 2048), an
attention width that differs from hidden, any vocabulary and four weight formats, and rca_lm.hip picks kernels and template
instances BY SHAPE: the prefill route (128-token tiles / 32-token tiles / the exact GEMV passes), the chunk count NIT of the down
projection, the attention instances <G> and <G, TEAMS>, the k-split form of every 128-row GEMM.  Every case below is a 2-layer
model with a vocabulary of 1-2 k (the fp32 oracle follows it in seconds) that is there to REACH one of those choices; `route`,
`nit` and `reaches` say which, and the CPU test checks the claims against a Python restatement of the library's rules (the
functions at the end of this file; the GPU test additionally asks the library itself, rca_lm_prefill_route).

Weights are model_path="random:<name>" (device-generated from the counter hash) and are regenerated for the oracle by
oracle.lm_ref.random_weights, put through oracle/q8_ref.py / q4k_ref.py / an fp16 round trip for the quantised formats.
"""
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

INIT_STD = 0.05
TOL_EXACT = 1e-3      # decode on a cache the exact GEMV passes built (test_lm_gpu.py's q8_0 / f16 / Q4_K decode bound)
TOL_TILE = 2e-3       # decode on a cache a tile route built (test_mid_size_..., test_q8_0_..., test_f16_..., test_q4_k_...)
FORMATS = ("bf16", "f16", "q8_0", "q4_k")
ROUTES = ("gemv", "tile32", "gemm128")     # rca_lm_prefill_route's 0 / 1 / 2

# the library's limits (rca_lm.hip)
LM_KSLICE, LM_MAXSPLIT, LM_MAXM, LM_TILE32, LM_PREFILL_MIN, ATT_KEYS = 2048, 4, 1024, 32, 8, 256


@dataclass(frozen=True)
class ShapeCase:
    name: str
    hidden: int
    n_heads: int
    n_kv_heads: int
    ffn: int
    vocab: int
    formats: Tuple[str, ...]
    route: str                      # with MFMA prefill switched ON (the default), for every format of the case
    reaches: str
    seed: int
    n_ctx: int = 1024
    prompt: int = 300               # prefill length of the oracle comparison (crosses the 256-key split)
    long_prompt: Optional[int] = None   # a second, longer prefill whose first pass is LM_MAXM tokens (flash TEAMS instance)
    flash: Optional[Tuple[int, int]] = None   # (G, TEAMS) the long prefill's first pass reaches on a 256-CU device

    @property
    def G(self):
        return self.n_heads // self.n_kv_heads

    @property
    def AO(self):
        return self.n_heads * 64

    @property
    def QKV(self):
        return (self.n_heads + 2 * self.n_kv_heads) * 64

    def config(self):
        from realtime_codec_agent_amd.llm import LMConfig
        return LMConfig(vocab_size=self.vocab, hidden=self.hidden, n_layers=2, n_heads=self.n_heads, n_kv_heads=self.n_kv_heads,
                        head_dim=64, ffn=self.ffn)

    def ids(self) -> np.ndarray:
        """n_ctx token ids: the longest prompt, the decode steps up to 520 keys and, for the ragged-context case, a full cache"""
        return np.random.default_rng(1000 + self.seed).integers(0, self.vocab, self.n_ctx).astype(np.int64)


CASES = (
    ShapeCase("g1_tile32", 192, 3, 3, 320, 1001, ("bf16",), "tile32",
              "lm_enqueue_prefill_tile (lm_gemm_mfma_kernel x 3 epilogues, lm_split_bf16_kernel); attention <1>; odd vocabulary; K = 24 / 40 chunks", 31),
    ShapeCase("g1_fallback", 192, 3, 3, 320, 1000, ("q8_0", "f16"), "gemv",
              "no tile route (not bf16, hidden % 128 != 0): the GEMV passes although MFMA prefill is on; q8_0 32-blocks at K = 6 / 10 blocks", 32),
    ShapeCase("h136_fallback", 136, 2, 1, 264, 777, ("bf16",), "gemv",
              "hidden % 64 != 0: fallback; K = 17 and 33 chunks (a wave partly idle); AO 128 != hidden; G = 2; odd vocabulary", 33),
    ShapeCase("g2_tile32", 320, 4, 2, 448, 1024, ("bf16",), "tile32", "32-token tiles with AO 256 != hidden 320, G = 2", 34),
    ShapeCase("g4_tile32", 192, 4, 1, 320, 1024, ("bf16",), "tile32", "32-token tiles at the deployed group size G = 4 (AO 256, QKV 384)", 35),
    ShapeCase("g4_fallback", 192, 4, 1, 320, 1024, ("q8_0",), "gemv", "the GEMV fallback at G = 4", 36),
    ShapeCase("g1_gemm128_ffn6144", 1024, 16, 16, 6144, 2048, FORMATS, "gemm128",
              "128-token tiles at G = 1; nit == 3 (NIT = 4 instance, short last chunk) in every format; lm_attn_flash_kernel<1, 2>", 37,
              n_ctx=1280, long_prompt=1100, flash=(1, 2)),
    ShapeCase("g2_gemm128_ffn4096", 1024, 16, 8, 4096, 2048, ("bf16",), "gemm128",
              "128-token tiles at G = 2; nit == 2; lm_attn_flash_kernel<2, 2>", 38, n_ctx=1280, long_prompt=1100, flash=(2, 2)),
    ShapeCase("g4_k768", 768, 12, 3, 768, 1536, ("q4_k", "q8_0"), "gemm128",
              "Q4_K 256-blocks / q8_0 32-blocks at K = 3 x 256 (not a power of two); 128-token tiles at G = 4", 39),
    ShapeCase("g1_k768", 768, 12, 12, 768, 1536, ("q4_k",), "gemm128", "Q4_K at K = 768 with G = 1 (QKV 2304)", 40),
    ShapeCase("nctx700", 192, 3, 3, 320, 1001, ("bf16",), "tile32",
              "n_ctx 700 (n_ctx_pad 768): the context limit falls inside the last attention split", 41, n_ctx=700),
    ShapeCase("g1_h2048_ffn8192", 2048, 32, 32, 8192, 2048, ("bf16",), "gemm128",
              "widest hidden at G = 1; nit == 4; lm_attn_flash_kernel<1, 4>", 42, n_ctx=1280, long_prompt=1100, flash=(1, 4)),
    ShapeCase("g2_h2048", 2048, 32, 16, 2048, 2048, ("bf16",), "gemm128",
              "widest hidden at G = 2; lm_attn_flash_kernel<2, 4>", 43, n_ctx=1280, long_prompt=1100, flash=(2, 4)),
)
BY_NAME = {c.name: c for c in CASES}
CASE_FORMATS = tuple((c.name, f) for c in CASES for f in c.formats)


# ------------------------------------------------------------------ the library's rules, restated
def cdiv(a: int, b: int) -> int:
    return -(-a // b)


def rejected(c: ShapeCase, fmt: str) -> Optional[str]:
    """lm_check_cfg and the row rules of the packed formats (RawMat::alloc): None when rca_lm_create accepts the shape"""
    if c.n_kv_heads < 1 or c.n_heads % c.n_kv_heads:
        return "n_heads must be a multiple of n_kv_heads"
    if c.G not in (1, 2, 4):
        return "query group size"
    if c.hidden % 8 or c.ffn % 8 or c.AO % 8:
        return "hidden / ffn must be multiples of 8"
    if c.hidden > LM_KSLICE or c.AO > LM_KSLICE:
        return "hidden too wide"
    if c.ffn > LM_KSLICE * LM_MAXSPLIT or (c.ffn > LM_KSLICE and c.ffn % LM_KSLICE):
        return "ffn"
    if c.vocab < 2 or c.n_ctx < 2:
        return "bad sizes"
    block = {"q8_0": 32, "q4_k": 256}.get(fmt, 1)      # row lengths: hidden (qkv, gate/up, head), AO (o), ffn (down)
    if c.hidden % block or c.AO % block or c.ffn % block:
        return f"{fmt} rows must be multiples of {block}"
    rows = {"q8_0": 2, "q4_k": 4}.get(fmt, 1)          # the packed layouts interleave row pairs / quads: lm_head's N is the vocabulary
    if c.vocab % rows:
        return f"{fmt} matrices need a multiple of {rows} rows"
    return None


def can_gemm128(c: ShapeCase) -> bool:
    """lm_can_gemm128 (one format per model: no separate V segment)"""
    return c.hidden % 128 == 0 and c.QKV % 128 == 0 and (2 * c.ffn) % 128 == 0 and c.AO % 32 == 0 and c.ffn % 32 == 0


def route(c: ShapeCase, fmt: str, mfma_prefill: bool = True) -> str:
    """lm_prefill_route: what an eval of more than LM_PREFILL_MIN tokens runs on"""
    if not mfma_prefill:
        return "gemv"
    if can_gemm128(c):
        return "gemm128"
    if fmt == "bf16" and c.hidden % 64 == 0 and c.AO % 64 == 0 and c.ffn % 64 == 0:
        return "tile32"
    return "gemv"


def gemv_nit(K: int) -> int:
    """launch_gemv_q: 16-byte chunks (8 values) per lane and wave, four waves along K"""
    return cdiv(cdiv(K >> 3, 4), 64)


def flash_teams(c: ShapeCase, M: int, n_cus: int) -> int:
    """launch_attention_flash_g: teams per workgroup for a prefill pass of M tokens on a device with n_cus compute units"""
    ntiles = cdiv(M * c.G, 32)
    if c.n_kv_heads * cdiv(ntiles, 4) >= n_cus:
        return 4
    if c.n_kv_heads * cdiv(ntiles, 2) >= n_cus:
        return 2
    return 1


def first_pass(c: ShapeCase, fmt: str, n: int) -> int:
    """tokens of the first pass of an n-token prefill"""
    r = route(c, fmt)
    return min(n, {"gemm128": LM_MAXM, "tile32": LM_TILE32, "gemv": 2}[r])


# ------------------------------------------------------------------ oracle weights
def oracle_weights(c: ShapeCase, fmt: str) -> dict:
    """the values the device holds for weight_format=fmt, as LMRef takes them"""
    from oracle import lm_ref, q4k_ref, q8_ref
    w = lm_ref.random_weights(c.config(), c.seed, INIT_STD)
    if fmt == "q8_0":
        return q8_ref.quantized_model(w)
    if fmt == "q4_k":
        return q4k_ref.quantized_model(w)
    if fmt == "f16":
        f32 = lambda v: (v.astype(np.uint32) << 16).view(np.float32)
        return {k: (f32(v).astype(np.float16).astype(np.float32) if (k.endswith("_proj.weight") or k == "lm_head.weight") else v)
                for k, v in w.items()}
    return w


def bound(want: np.ndarray, tol: float) -> float:
    """the project's normalisation of a logit tolerance"""
    return tol * max(1.0, float(np.abs(want).max()))
