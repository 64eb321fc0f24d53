"""CPU measurement behind the tolerance of tests/test_kv_q8_gpu.py::test_end_to_end_logits (run: python tests/kv_q8_spread.py).

Device and oracle K / V rows may differ by an fp16 ulp BEFORE the quantiser (the projections round differently), and one ulp can
flip an int8 step of a block.  How far that moves the logits is measured here without a GPU: Q8KVRef against a Q8KVRef whose
pre-quantisation rows are moved by -1 / 0 / +1 fp16 ulp at random, on the models, prompts and steps the GPU test uses; the figure is
max |dlogit| / max(1, |logit|max) over the prompt's last position and the decode steps, the largest of 5 seeds."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kv_q8_ref as kr  # noqa: E402
import lm_shape_cases as sc  # noqa: E402

E2E_CASES = {"gemv": ("g1_fallback", "q8_0"), "tile32": ("g4_tile32", "bf16"), "gemm128": ("g4_k768", "q8_0")}
E2E_PROMPT, E2E_STEPS = 300, 4
# measured with this file (5 seeds), in units of max(1, |logit|max)
SPREAD = {"gemv": 3.38e-3, "tile32": 4.49e-3, "gemm128": 2.05e-2}


def member_ids(case, s: int) -> np.ndarray:
    """prompt + step tokens of session s of a case (sessions of a batch / group read different stretches of the case's ids)"""
    return case.ids()[40 * s: 40 * s + E2E_PROMPT + E2E_STEPS]


def ref_logits(ref, ids) -> np.ndarray:
    """[1 + E2E_STEPS, V]: the prompt's last logits, then one row per single-token step"""
    ref.reset()
    rows = [ref.eval(ids[:E2E_PROMPT], last_only=True)[-1].numpy()]
    for t in ids[E2E_PROMPT:]:
        rows.append(ref.eval([int(t)])[-1].numpy())
    return np.stack(rows)


def measure(route: str, seeds=range(5)) -> float:
    name, fmt = E2E_CASES[route]
    c = sc.BY_NAME[name]
    w = sc.oracle_weights(c, fmt)
    ids = member_ids(c, 0)
    ref = kr.Q8KVRef(c.config(), w)
    want = ref_logits(ref, ids)
    worst = 0.0
    for seed in seeds:
        jit = kr.Q8KVRef(c.config(), w)
        jit.jitter = np.random.default_rng(9000 + seed)
        got = ref_logits(jit, ids)
        worst = max(worst, float(np.abs(got - want).max()) / max(1.0, float(np.abs(want).max())))
    return worst


if __name__ == "__main__":
    for r in E2E_CASES:
        print(f"{r:8s} {E2E_CASES[r][0]:12s} spread {measure(r):.3e}", flush=True)
