"""CPU measurement behind the tolerance of tests/test_kv_q8_shift_gpu.py::test_logits_on_a_shifted_q8_cache (run: python
tests/kv_q8_shift_spread.py).

Device and oracle start that test from identical cache rows (the device's own blocks, de-quantised).  From there on their fp16 rows
may differ by an ulp BEFORE a quantiser -- the rotated keys of a shift (f32 on the device, float64 in the oracle) and the new K / V
rows of the passes that follow -- and one ulp can flip an int8 step of a block.  How far that moves the logits is measured here
without a GPU: the oracle of the test against the same oracle whose pre-quantisation rows (rotated and new) are moved by -1 / 0 / +1
fp16 ulp at random, on the models, tokens and steps the GPU test uses; the figure is max |dlogit| / max(1, |logit|max) over the four
compared logit rows, the largest of 5 seeds."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kv_q8_ref as kr  # noqa: E402
import kv_q8_shift_ref as qs  # noqa: E402
import kv_q8_spread as ks  # noqa: E402
import lm_shape_cases as sc  # noqa: E402

CASES = ks.E2E_CASES                       # route -> (model, weight format)
PROMPT = 300
REMOVE_1, REMOVE_2 = (20, 120), (5, 60)    # 300 -> 200 positions (a tail of 180 rows), ..., 242 -> 187
# measured with this file (5 seeds), in units of max(1, |logit|max)
SPREAD = {"gemv": 2.11e-3, "tile32": 2.63e-3, "gemm128": 1.13e-2}


def sequence(ids, evaluate, remove):
    """the steps after the prompt: remove, a 2-token decode, a 40-token prefill, a second remove, another decode; evaluate(tokens)
    returns the last position's logits.  -> the four logit rows [3, V] ... in order (decode, prefill, decode)"""
    n = PROMPT
    rows = []
    remove(*REMOVE_1)
    rows.append(evaluate(ids[n:n + 2]))
    rows.append(evaluate(ids[n + 2:n + 42]))
    remove(*REMOVE_2)
    rows.append(evaluate(ids[n + 42:n + 44]))
    return np.stack(rows)


def oracle_sequence(ref, ids, jitter=None):
    """ref: a Q8KVRef holding the prompt's cache"""
    ref.jitter = jitter
    try:
        return sequence(ids, lambda t: ref.eval([int(x) for x in t], last_only=True)[-1].numpy(),
                        lambda p0, p1: qs.kv_remove_q8_ref(ref, p0, p1, jitter=jitter))
    finally:
        ref.jitter = None


def measure(route: str, seeds=range(5)) -> float:
    name, fmt = CASES[route]
    c = sc.BY_NAME[name]
    w = sc.oracle_weights(c, fmt)
    ids = c.ids().tolist()[:PROMPT + 44]

    def run(jitter):
        ref = kr.Q8KVRef(c.config(), w)
        ref.eval(ids[:PROMPT], last_only=True)
        return oracle_sequence(ref, ids, jitter)

    want = run(None)
    worst = 0.0
    for seed in seeds:
        got = run(np.random.default_rng(9100 + seed))
        worst = max(worst, float(np.abs(got - want).max()) / max(1.0, float(np.abs(want).max())))
    return worst


if __name__ == "__main__":
    for r in CASES:
        print(f"{r:8s} {CASES[r][0]:12s} spread {measure(r):.3e}", flush=True)
