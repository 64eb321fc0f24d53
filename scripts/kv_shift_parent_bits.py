"""Bit-identity of the fp16 context shift across two builds of the library: the cache rows rca_lm_kv_remove and rca_lm_kv_remove_many
(own routing and held on the staged route) leave on the model g4_tile32 of tests/lm_shape_cases.py at the spans of
tests/test_kv_shift_gpu.py, one SHA-256 per (call, span, layer, tensor).
    python scripts/kv_shift_parent_bits.py                       prints the lines of the library in use (RCA_LIB_PATH or the in-tree one)
    python scripts/kv_shift_parent_bits.py --against OTHER.so    runs itself again in a fresh process over OTHER.so, compares the two
                                                                 outputs line by line and exits 1 unless all lines are equal
The rotation of the fp16 unit and of the q8_0 unit is one helper (lm_kv_unrotate, rca_lm.hip); this is the check that introducing it
left the fp16 rows what they were."""
import hashlib, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SPANS = [(900, 20, 21), (900, 7, 44), (600, 10, 400), (300, 0, 100), (520, 256, 512), (300, 100, 300), (300, 50, 50)]


def lines():
    import numpy as np
    import lm_shape_cases as sc
    from realtime_codec_agent_amd.llm import LlamaForAlternatingCodeChannels, kv_remove_many
    c = sc.BY_NAME["g4_tile32"]
    parent = LlamaForAlternatingCodeChannels(model_path="random:g4_tile32", config=c.config(), n_ctx=c.n_ctx, random_seed=c.seed, init_std=sc.INIT_STD, device=0)
    twins = [LlamaForAlternatingCodeChannels(model_path=parent.model_path, n_ctx=c.n_ctx, share_weights_with=parent, device=0) for _ in SPANS]
    ids = c.ids().tolist()
    h = lambda a: hashlib.sha256(np.ascontiguousarray(a).view(np.uint16).tobytes()).hexdigest()[:16]
    out = []
    for kind in ("kv_remove", "kv_remove_many", "kv_remove_many_staged"):
        for m, (n, _, _) in zip(twins, SPANS):
            m.reset()
            m.eval(ids[:n])
        if kind == "kv_remove":
            for m, (n, p0, p1) in zip(twins, SPANS):
                m.kv_remove(p0, p1)
        else:
            kv_remove_many(twins, [(p0, p1) for _, p0, p1 in SPANS], staged_only=kind.endswith("staged"))
        for m, (n, p0, p1) in zip(twins, SPANS):
            assert m.n_tokens == n - (p1 - p0)
            for l in range(c.config().n_layers):
                k, v = m.kv_read(l, 0, n)          # the stale rows above the new end included
                out.append(f"{kind} n={n} [{p0}, {p1}) layer {l}: K {h(k)} V {h(v)}")
    return out


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--against":
        mine = lines()
        env = dict(os.environ, RCA_LIB_PATH=os.path.abspath(sys.argv[2]))
        theirs = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, check=True, capture_output=True, text=True, timeout=300).stdout.splitlines()
        same = sum(a == b for a, b in zip(mine, theirs))
        for a, b in zip(mine, theirs):
            if a != b:
                print("DIFFERENT:", a, "|", b)
        print(f"{same} of {len(mine)} lines identical to {sys.argv[2]} ({len(theirs)} lines there)")
        sys.exit(0 if same == len(mine) == len(theirs) else 1)
    print("\n".join(lines()))
