"""Bit-identity A/B of the weight LOAD path of two builds of the library (ab_logits.py generates its weights on the device and never
loads a block): one small GGUF model per file kind, written with tests/gguf_writer.py and the writers of the file tests, loaded with its
blocks packed and its embedding table quantised, then one SHA-256 per line of what the loaded arrays compute.  Run once per library
and compare the outputs:
    RCA_LIB_PATH=/tmp/librca_hip_parent.so python scripts/ab_weights.py > a.txt; python scripts/ab_weights.py > b.txt; diff a.txt b.txt
Lines per model: the logits of a 40-token eval on the exact route and (where the shape allows them) on the 128-token tiles, of one
2-token step, of the same eval after mask_head_rows(0, 64), and rca_lm_weight_format's two outputs."""
import hashlib, os, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import gguf_writer as gw
import lm_iq4_cases, lm_q40_cases, lm_q5k_cases, lm_split_v_case
from realtime_codec_agent_amd.gguf import load_llama_gguf, read_gguf
from realtime_codec_agent_amd.llm import LlamaForAlternatingCodeChannels


def plain(matrix_type):
    def write(path):
        cfg = lm_q40_cases.file_config("q4_0")
        gw.write_llama_gguf(path, cfg, lm_q40_cases.f32_weights(cfg, 6), matrix_type=matrix_type)
    return write


# file kind -> writer(path)
KINDS = {"f32": plain(gw.F32), "f16": plain(gw.F16), "bf16": plain(gw.BF16), "q8_0": plain(gw.Q8_0), "q4_k": plain(gw.Q4_K),
         "q4_k_m": lm_split_v_case.write_file, "q6_k": plain(gw.Q6_K), "q5_k_m": lambda p: lm_q5k_cases.write_file("q5_k_m", p),
         "q4_0_mix": lambda p: lm_q40_cases.write_file("q4_0_mix", p), "iq4_nl": lambda p: lm_iq4_cases.write_file("iq4_nl", p),
         "iq4_xs_mix": lambda p: lm_iq4_cases.write_file("iq4_xs_mix", p)}
h = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]

for kind, write in KINDS.items():
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, kind + ".gguf")
        write(path)
        cfg, w, _ = load_llama_gguf(path)
        w["model.embed_tokens.weight"] = read_gguf(path, keep_q8_0=True)[1]["token_embd.weight"]   # as the file holds it: the device de-quantises it
        llm = LlamaForAlternatingCodeChannels(config=cfg, weights=w, n_ctx=512, device=0)
    kinds = sorted({type(v).__name__ for v in w.values()})
    ids = np.random.default_rng(4).integers(0, cfg.vocab_size, 42).tolist()

    def eval40(tiles):
        llm.set_mfma_prefill(tiles)
        llm.reset()
        llm.eval(ids[:40])
        return llm.prefill_route(), h(llm._scores[-1])

    print(f"{kind} tensors {' '.join(kinds)}")
    print(f"{kind} format {llm.weight_format} bytes_per_step {llm.weight_bytes_per_step()}")
    print(f"{kind} eval40 exact ({'%s) %s' % eval40(False)}")
    route, digest = eval40(True)
    if route != "gemv":
        print(f"{kind} eval40 tiles ({route}) {digest}")
    llm.set_mfma_prefill(False)
    llm.init_sampler_for_generate(top_k=100, top_p=1.0, min_p=0.0, temp=1.0, seed=9)
    tok = llm.step(ids[40:42])
    print(f"{kind} step2 token {tok} {h(llm._scores[-1])}")
    llm.mask_head_rows(0, 64)
    route, digest = eval40(False)
    assert not llm._scores[-1][:64].any() and llm._scores[-1][64:].any()
    print(f"{kind} eval40 masked rows 0..63 ({route}) {digest}")
    llm.close()
