"""Cases, inputs and references for the layer-by-layer tests of the f32 encoder (test_encoder_layers_cpu.py, test_encoder_layers_gpu.py).

A case is ONE encoder layer (0 = enc.conv_in, 1..n = enc.down.{0..n-1}, n + 1 = enc.conv_out) of one config on one input shape, run by
rca_codec_encoder_layer_tap as an encode pass launches it: on route 0 (the throughput launch) or route 1 (the lat_mode launch of the
streaming tail), under one kernel variant, with the flags a pass would set (1: the input holds LeakyReLU(x) already, 2: the launch
stores LeakyReLU(y), 4: the input is PCM and the launch is conv_in fused into the first strided layer), over a view of the last
layer's trailing columns or the whole row, and under the environment switches a pass reads per call.  Every case names the kernel class
the launch logic of csrc/rca_codec.hip must pick for it.  That logic is restated here as plain inequalities (enc_route0_class,
enc_route1_class, fuse_class, handoff, view_ok): the CPU test checks the tables against them, the GPU test checks what the tap reports.

References, in rising distance from the kernels:
  * the C oracle: oracle.codec.conv1d per layer and OracleCodec.encode(tap_layer=0 / 1) for the launches that read PCM -- the fma order
    every kernel must reproduce bit for bit.  conv1d(x, pre=True) == conv1d(max(x, slope x), pre=False) bit for bit, so an activated
    input (flag 1) has the same reference as the plain one, and flag 2 expects max(y, slope y);
  * ref64: the layer in float64 numpy with the per-element magnitude m = |b| + sum |w| |x|;
  * fma_bound = (K + 1) u m, K = Cin k, u = 2^-24: derived in tests/dec_cases.py (Higham 3.1), not measured.
"""
import functools
import zlib
from collections import namedtuple

import numpy as np

from realtime_codec_agent_amd import _native as N
from realtime_codec_agent_amd.codec_model import CodecConfig, init_codec_weights, tiny_codec_config

U = 2.0 ** -24
LAT_MAX_FRAMES = 64            # RCA_LAT_MAX_FRAMES
LDS_BUDGET = 152 * 1024        # RCA_LDS_BUDGET
GMAC_ALL_ROWS = 1.0e8          # a case under ~0.1 GMAC runs every batch row through the CPU oracle

CHAIN, M32x32, M64x32, M32x64, M64x64, WS, BF16, WIDE, FIRST = (N.KCLASS_CHAIN, N.KCLASS_MFMA_32x32, N.KCLASS_MFMA_64x32,
                                                                 N.KCLASS_MFMA_32x64, N.KCLASS_MFMA_64x64, N.KCLASS_WS, N.KCLASS_BF16,
                                                                 N.KCLASS_MFMA_OTHER, N.KCLASS_FIRST_MFMA)
LDS1, LDS4 = N.KCLASS_LDS + 1, N.KCLASS_LDS + 4
MIXED = N.KCLASS_MIXED
# every class include/rca.h documents for an encoder layer in the default arithmetic (mfma mode 0).  The latency kernel of a plain conv
# has 4 waves or, for Cout < 4, one; LDS + 2 is a transposed (decoder) layer's.
ENCODER_CLASSES = {CHAIN, M32x32, M64x32, M32x64, M64x64, WS, WIDE, FIRST, LDS1, LDS4, M32x64 | MIXED, M64x64 | MIXED}

# input channels per K chunk of conv1d_mfma_kernel by kernel size (conv_cic): a layer whose Cin is a multiple runs the whole-chunk
# instantiation, which alone has the mixed grid
CIC = {4: 4, 8: 4, 10: 4, 16: 2, 3: 8}
MFMA_KS = {(4, 2), (8, 4), (10, 5), (16, 8), (3, 1)}       # mfma_supported: only these layers get packed weights
FUSABLE = {(4, 2), (8, 4), (16, 8)}

# name -> (config, weight seed).  Small channel counts keep the CPU oracle quick; "full" is the shipped model.
#   odd:    the config of test_codec_gpu.py: partial K chunks on every strided layer but the last two, conv_out with Cin % 16 != 0
#   f84 / f168: a k8s4 / k16s8 first strided layer behind a 7-tap conv_in: the fused first layer on those kernels
#   k105:   a k10s5 first strided layer (never fused) behind conv_in_kernel<5>;  kin3: conv_in_kernel<3>
#   s3:     a stride the matrix kernels do not have (k6s3): no packed weights, the scalar chain under every variant.  (Every layer
#           with one of the four strides is packed whatever Cin * k is: the tiny config's 4 -> 8 k4s2 layer, Cin k = 16, runs on the
#           matrix pipe.)
#   lat64:  conv_out 16 -> 64: wide enough for the 64 x 32 tiles of the k = 3 layer
#   c2:     two channels everywhere: Cout < 4 picks the one-wave latency kernel, Cin < 8 lets it take the k16s8 layer
_CONFIGS = {
    "full": (lambda: CodecConfig(), 0),
    "tiny": (lambda: tiny_codec_config(), 0),
    "odd": (lambda: tiny_codec_config(channels=(6, 10, 12, 20, 36), latent_dim=24, name="odd"), 3),
    "f84": (lambda: tiny_codec_config(strides=(4, 2, 5, 8), channels=(8, 16, 16, 16, 16), name="f84"), 4),
    "f168": (lambda: tiny_codec_config(strides=(8, 5, 4, 2), name="f168"), 5),
    "k105": (lambda: tiny_codec_config(strides=(5, 8, 2, 4), k_in=5, name="k105"), 6),
    "kin3": (lambda: tiny_codec_config(k_in=3, name="kin3"), 7),
    "s3": (lambda: tiny_codec_config(strides=(2, 3, 5, 8), name="s3"), 8),
    "lat64": (lambda: tiny_codec_config(latent_dim=64, name="lat64"), 9),
    "c2": (lambda: tiny_codec_config(channels=(2, 2, 2, 2, 2), latent_dim=2, name="c2"), 10),
}


@functools.lru_cache(maxsize=None)
def config(name):
    """(cfg, weights) of a named config; "full" and "tiny" are what the full_codec / tiny_codec fixtures hold."""
    make, seed = _CONFIGS[name]
    cfg = make()
    return cfg, init_codec_weights(cfg, seed=seed)


def n_layers(name):
    return len(config(name)[0].encoder_layers())


def layer_of(name, layer):
    return config(name)[0].encoder_layers()[layer]


def frame_mult(name, layer):
    """input samples per frame at this layer: the strides still to come (the hop for conv_in and the first strided layer)"""
    m = 1
    for ly in config(name)[0].encoder_layers()[max(layer, 1):]:
        m *= ly["s"]
    return m


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------ the launch logic, restated
def waves(ly, B, cols):
    """waves of 64 x 64 a launch of B rows of `cols` output columns would take (waves_big of launch_conv_mfma)"""
    return cdiv(B * cols, 64) * cdiv(ly["cout"], 64)


def packed(ly):
    return (ly["k"], ly["s"]) in MFMA_KS and ly["name"] != "enc.conv_in"


def mfma_ok(ly, variant):
    """mfma_conv_ok, without its 32-bit offset limits (no case here is near them)"""
    return variant >= 1 and packed(ly)


def whole_chunks(ly):
    return ly["k"] in CIC and ly["cin"] % CIC[ly["k"]] == 0


def enc_route0_class(ly, B, Lin, variant, balance=True, cols=None):
    """the low bits of the class run_conv reports for layer ly (not conv_in) on route 0; cols: the view, else Lin / s"""
    cols = Lin // ly["s"] if cols is None else cols
    if not mfma_ok(ly, variant):
        return CHAIN
    w = waves(ly, B, cols)
    if variant == 2 and w >= 1024:
        return WS
    big_min = 3072 if (ly["k"] >= 8 and balance and whole_chunks(ly)) else 8192
    if w >= big_min:
        return M64x64
    if w >= 2048:
        return M32x64
    if ly["k"] == 3 and ly["cout"] >= 64 and w >= 1024:
        return M64x32
    return M32x32


def may_mix(ly, kclass):
    """the launches launch_conv_cfg hands to launch_conv_balanced: k >= 8, whole chunks, 64 columns per wave"""
    return ly["k"] >= 8 and whole_chunks(ly) and kclass in (M32x64, M64x64)


def plan_of(plan, ly, B, cols, kclass):
    """conv_balance_parse for a launch of class kclass: (bulk column tiles, fine columns per wave) or None for the single-shape grid"""
    if plan is None or not may_mix(ly, kclass):
        return None
    bulk, fine = plan.split(":")
    fwn = {"32x64": 2, "32x32": 1}[fine]
    wm = 2 if kclass == M64x64 else 1
    if fwn >= wm * 2:
        return None
    total = cdiv(B * cols, 64)
    bulk = min(int(bulk), total) // 8 * 8
    return None if bulk >= total else (bulk, fwn * 32)


def view_chunk16(ly, B, view):
    """the 16-channel-chunk instance of the view (run_conv_launch): at most 1024 tiles of 32 x 32, Cin a multiple of 16"""
    return ly["k"] == 3 and cdiv(B * view, 32) * cdiv(ly["cout"], 32) <= 1024 and ly["cin"] % 16 == 0


def view_class(ly, B, Lin, view):
    return M32x32 if view_chunk16(ly, B, view) else enc_route0_class(ly, B, Lin, 1, cols=view)


def view_halo(ly):
    pad = (ly["k"] - ly["s"] + 1) // 2
    return cdiv(pad, ly["s"])


def view_ok(name, layer, B, Lin, view, variant=1):
    """enc_last_view with keep = view - halo: the last layer, the default variant's matrix kernel, a view shorter than the row"""
    ly = layer_of(name, layer)
    return layer == n_layers(name) - 1 and variant == 1 and mfma_ok(ly, variant) and view_halo(ly) < view < Lin // ly["s"]


def handoff(name, nxt, variant):
    """enc_handoff: layer `nxt` exists, is pre-activated and runs on conv1d_mfma_kernel of the default variant"""
    return variant == 1 and nxt < n_layers(name) and layer_of(name, nxt)["pre"] and mfma_ok(layer_of(name, nxt), variant)


def flags_ok(name, layer, flags, variant, fused_ok=False):
    """what rca_codec_encoder_layer_tap accepts: flag 1 needs the hand-off into `layer` from a layer that can store an activated
    output (layer >= 2), flag 2 the hand-off into layer + 1, flag 4 layer 1 and the fusion predicate"""
    if flags & 4 and (layer != 1 or flags & 1 or not fused_ok):
        return False
    if flags & 1 and not (layer >= 2 and handoff(name, layer, variant)):
        return False
    if flags & 2 and not (layer >= 1 and handoff(name, layer + 1, variant)):
        return False
    return True


def fuse_ok(name, B, T, variant):
    """enc_fuse01 for plain rows (32-bit offset limits left out)"""
    cfg = config(name)[0]
    e1 = layer_of(name, 1)
    L = cdiv(T, cfg.hop) * cfg.hop
    return variant >= 1 and cfg.k_in == 7 and (e1["k"], e1["s"]) in FUSABLE and L // e1["s"] >= 67


def fuse_class(name, B, T, variant, mfma_in=True):
    """the class of the fused first layer (the `fuse` branch of launch_conv_mfma; RCA_FUSE_WIDE at its default)"""
    cfg = config(name)[0]
    e1 = layer_of(name, 1)
    Lout = cdiv(T, cfg.hop) * cfg.hop // e1["s"]
    w = waves(e1, B, Lout)
    if variant == 2 and w >= 1024 and e1["k"] == 4:
        return WS
    if e1["k"] == 4 and w >= 8192:
        if mfma_in and Lout >= 131 and e1["cin"] == 32 and e1["cout"] % 64 == 0:
            return FIRST
        if Lout >= 131 and e1["cin"] % 2 == 0:
            return WIDE
    return M64x64 if w >= 8192 else M32x32


def enc_route1_class(name, layer, B, Lin, variant=1):
    """the latency launcher's own conditions (try_conv_lds); a shape it declines falls through to the route-0 launch, conv_in to
    conv_in_kernel"""
    ly = layer_of(name, layer)
    cin, cout, k, s = ly["cin"], ly["cout"], ly["k"], ly["s"]
    nw = 4 if cout >= 4 else 1
    if (k, s) not in MFMA_KS | {(7, 1)} or lds_columns(ly, Lin) is None or (cin >= 8 and 4 * k > 64):
        return CHAIN if layer == 0 else enc_route0_class(ly, B, Lin, variant)
    return N.KCLASS_LDS + nw


def lds_columns(ly, Lin):
    """NC of try_conv_lds: columns per workgroup after the LDS budget halved them; None when even one column does not fit"""
    cin, cout, k, s = ly["cin"], ly["cout"], ly["k"], ly["s"]
    nw = 4 if cout >= 4 else 1
    lds = lambda c: (((c * s + k - s + 6) & ~3) * (cin + 4) + nw * cin * k) * 4
    nc = min(64, Lin // s)
    while nc > 1 and lds(nc) > LDS_BUDGET:
        nc = (nc + 1) // 2
    return None if lds(nc) > LDS_BUDGET else nc


# ------------------------------------------------------------------------------------------------ the case tables
Case = namedtuple("Case", "group config layer route variant flags view B Lin kind kclass mixed env")
# B, Lin: the tap's input shape (Lin = T samples of PCM for layer 0 and flag 4).  kind: "normal", "signed", "imp_first", "imp_last".
# kclass: the low bits the tap must report; mixed: True / False where the launch must / must not be the mixed grid, None where the
# automatic plan decides (it depends on the device's SIMD count and the kernel's occupancy).
# env: ((name, value), ...) set around the call and restored.


def shape_for(name, layer, want_waves, cols=None):
    """(B, Lin) with B >= 3 rows, a row length that is no multiple of 64 and a whole number of frames, whose launch takes want_waves
    waves of 64 x 64 or the nearest count a whole number of frames gives: a threshold (a multiple of 1024) is met from above, within 8
    column tiles, every other count (a threshold less one tile) from below"""
    ly = layer_of(name, layer)
    mult = frame_mult(name, layer)
    per_frame = mult // ly["s"]                       # output columns per frame
    n_co = cdiv(ly["cout"], 64)
    assert want_waves % n_co == 0
    tiles, up = want_waves // n_co, want_waves % 1024 == 0
    best = None
    for B in (3, 5, 7, 9, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 53, 59, 61):
        f = tiles * 64 // (B * per_frame)
        for F in range(max(1, f - 2), f + 3):
            got = cdiv(B * F * per_frame, 64)
            off = got - tiles if up else tiles - got
            if 0 <= off < 8 and (F * per_frame) % 64 != 0 and (best is None or off < best[0]):
                best = (off, B, F * mult)
    assert best, (name, layer, want_waves)
    return best[1:]


def shape_waves(name, layer, B, Lin):
    ly = layer_of(name, layer)
    return waves(ly, B, Lin // ly["s"])


def _flag_sets(name, layer, variant):
    return [f for f in (0, 1, 2, 3) if flags_ok(name, layer, f, variant)]


def _env(**kw):
    return tuple(sorted((k, v) for k, v in kw.items() if v is not None))


# route 0 thresholds of the strided layers and conv_out: (config, layer, waves) at the threshold and one column tile below it
THRESHOLDS = [
    ("tiny", 1, 2048), ("tiny", 1, 2047), ("tiny", 1, 8192), ("tiny", 1, 8191),            # k4s2: no mixed grid, 64 x 64 from 8192
    ("tiny", 2, 2048), ("tiny", 2, 2047), ("tiny", 2, 3072), ("tiny", 2, 3071),            # k8s4, whole chunks: 64 x 64 from 3072
    ("tiny", 3, 2048), ("tiny", 3, 2047), ("tiny", 3, 3072), ("tiny", 3, 3071),            # k10s5
    ("tiny", 4, 2048), ("tiny", 4, 2047), ("tiny", 4, 3072), ("tiny", 4, 3071),            # k16s8
    ("odd", 2, 3072), ("odd", 2, 8191), ("odd", 2, 8192),                                  # k8s4, Cin = 10: partial chunks, 8192 again
    ("odd", 1, 2048), ("odd", 1, 2047),                                                    # k4s2, Cin = 6: partial chunks
    ("lat64", 5, 1024), ("lat64", 5, 1023), ("lat64", 5, 2048), ("lat64", 5, 2047), ("lat64", 5, 8192), ("lat64", 5, 8191),
    ("tiny", 5, 1024), ("odd", 5, 2048), ("odd", 5, 2047),                                 # k = 3 with Cout < 64: no 64 x 32
]
# RCA_CONV_BALANCE=0 twins of the balanced layers: the single-shape classes (64 x 64 only from 8192)
UNBALANCED = [("tiny", 2, 3072), ("tiny", 3, 3072), ("tiny", 4, 3072), ("tiny", 4, 2048)]
# forced seams: (config, layer, waves, plan).  The bulk column tiles times 64 columns fall inside a row (checked by the CPU test).
FORCED = [
    ("tiny", 2, 3072, "1000:32x64"), ("tiny", 2, 3072, "1000:32x32"), ("tiny", 2, 2048, "1000:32x32"),
    ("tiny", 3, 3072, "1000:32x64"), ("tiny", 3, 3072, "1000:32x32"), ("tiny", 3, 2048, "1000:32x32"),
    ("tiny", 4, 3072, "1000:32x64"), ("tiny", 4, 3072, "1000:32x32"), ("tiny", 4, 2048, "1000:32x32"),
    ("tiny", 2, 3072, "0:32x32"), ("tiny", 2, 3072, "3064:32x64"),                         # all fine tiles; the last 8 column tiles
]
SMALL_SHAPES = [(3, 1), (3, 3), (4, 7)]                      # (B, frames): one tile and less, tiles that straddle rows
SMALL_CONFIGS = ("tiny", "odd", "f84", "f168", "k105", "kin3", "s3", "lat64", "c2")
# the view of conv_out: (config, B, frames per row, view)
VIEWS = [
    ("tiny", 3, 9, 2), ("tiny", 3, 9, 8), ("tiny", 5, 70, 33),                             # keep + halo = 2; Lout - 1; a tile and a column
    ("tiny", 8, 4100, 4096), ("tiny", 8, 4100, 4097),                                      # 1024 tiles of 32 x 32 and 1025
    ("odd", 3, 9, 2), ("odd", 5, 70, 33), ("lat64", 3, 70, 69),                            # Cin = 36: never the 16-channel chunk
    ("full", 40, 100, 6), ("full", 256, 100, 6),                                           # the benchmark's: 6 columns of 100
]
ROUTE1_FRAMES = [(1, 1), (1, 2), (1, 3), (1, 8), (1, 9), (1, 64), (3, 5), (8, 8), (64, 1)]   # (B, F), B * F <= LAT_MAX_FRAMES
# (no (k, s) of the matrix kernels is declined by try_conv_lds: its `Cin >= 8 && 4 k > 64` needs k > 16.  s3's k6s3 layer is the
#  one shape it has no instance for; that layer falls through to the launch of route 0, the scalar chain.)
ROUTE1_CONFIGS = ("tiny", "odd", "c2", "k105", "kin3", "s3")
ROUTE1_FULL = [(1, 1), (1, 8), (1, 9), (2, 3)]              # the shipped model: layer 3 (128 channels, k10s5) halves its columns
# the fused first layer: (config, B, T, variant, RCA_FUSE_MFMA_IN)
FUSED = [
    ("full", 33, 32000, 1, None), ("full", 33, 32000, 1, "0"), ("full", 3, 1700, 1, None), ("full", 5, 26001, 2, None),
    ("tiny", 33, 32000, 1, None), ("tiny", 33, 31700, 1, None), ("tiny", 3, 1700, 1, None), ("tiny", 3, 134, 1, None),
    ("f84", 9, 233600, 1, None), ("f84", 9, 233000, 1, None), ("f84", 3, 1700, 1, None), ("f84", 3, 268, 1, None),
    ("f168", 9, 466240, 1, None), ("f168", 9, 465800, 1, None), ("f168", 3, 1700, 1, None), ("f168", 3, 536, 1, None),
]


@functools.lru_cache(maxsize=None)
def cases():
    out = []

    def add(group, name, layer, route, variant, flags, view, B, Lin, kind, kclass, mixed=False, **env):
        out.append(Case(group, name, layer, route, variant, flags, view, B, Lin, kind, kclass, mixed, _env(**env)))

    # conv_in alone: conv_in_kernel<7 / 5 / 3> on ragged rows, and the impulses at the row edges
    for name in ("tiny", "k105", "kin3", "full"):
        hop = config(name)[0].hop
        for B, T in ((3, 2 * hop - 37), (4, hop), (3, 1)):
            add("conv_in", name, 0, 0, 1, 0, 0, B, T, "normal", CHAIN)
        for kind in ("imp_first", "imp_last"):
            add("conv_in", name, 0, 0, 1, 0, 0, 2, 2 * hop - 37, kind, CHAIN)
    # every later layer of every small config at small shapes: variants 0 and 1, every flag combination the pass can set
    for name in SMALL_CONFIGS:
        for layer in range(1, n_layers(name)):
            ly, mult = layer_of(name, layer), frame_mult(name, layer)
            for variant in (0, 1):
                for B, F in SMALL_SHAPES:
                    for flags in _flag_sets(name, layer, variant):
                        add("small", name, layer, 0, variant, flags, 0, B, F * mult, "signed" if flags else "normal",
                            enc_route0_class(ly, B, F * mult, variant))
                for kind in ("imp_first", "imp_last"):
                    add("small", name, layer, 0, variant, 0, 0, 2, 3 * mult, kind, enc_route0_class(ly, 2, 3 * mult, variant))
    # each class at its threshold and one column tile below
    for name, layer, w in THRESHOLDS:
        ly = layer_of(name, layer)
        B, Lin = shape_for(name, layer, w)
        kclass = enc_route0_class(ly, B, Lin, 1)
        for flags in _flag_sets(name, layer, 1):
            add("threshold", name, layer, 0, 1, flags, 0, B, Lin, "signed" if flags else "normal", kclass,
                None if may_mix(ly, kclass) else False)
    for name, layer, w in UNBALANCED:
        ly = layer_of(name, layer)
        B, Lin = shape_for(name, layer, w)
        for flags in (0, 3):
            add("unbalanced", name, layer, 0, 1, flags, 0, B, Lin, "signed" if flags else "normal",
                enc_route0_class(ly, B, Lin, 1, balance=False), False, RCA_CONV_BALANCE="0")
    for name, layer, w, plan in FORCED:
        ly = layer_of(name, layer)
        B, Lin = shape_for(name, layer, w)
        kclass = enc_route0_class(ly, B, Lin, 1)
        for flags in (0, 3):
            add("forced", name, layer, 0, 1, flags, 0, B, Lin, "signed" if flags else "normal", kclass,
                plan_of(plan, ly, B, Lin // ly["s"], kclass) is not None, RCA_CONV_BALANCE_PLAN=plan)
    # variant 2: the warp-specialised kernel from 1024 waves
    for name, layer in (("tiny", 2), ("tiny", 5), ("lat64", 5)):
        for w in (1024, 1023):
            B, Lin = shape_for(name, layer, w)
            add("ws", name, layer, 0, 2, 0, 0, B, Lin, "normal", enc_route0_class(layer_of(name, layer), B, Lin, 2))
    # the view of the last layer
    for name, B, F, view in VIEWS:
        layer = n_layers(name) - 1
        ly = layer_of(name, layer)
        for flags in _flag_sets(name, layer, 1):
            add("view", name, layer, 0, 1, flags, view, B, F, "signed" if flags else "normal", view_class(ly, B, F, view))
    # the fused first layer, with and without the activated store
    for name, B, T, variant, mfma_in in FUSED:
        for flags in (4, 6):
            if flags_ok(name, 1, flags, variant, fuse_ok(name, B, T, variant)):
                add("fused", name, 1, 0, variant, flags, 0, B, T, "signed", fuse_class(name, B, T, variant, mfma_in != "0"),
                    False, RCA_FUSE_MFMA_IN=mfma_in)
    # route 1: the streaming tail
    for name in ROUTE1_CONFIGS:
        hop = config(name)[0].hop
        for layer in range(n_layers(name)):
            mult = frame_mult(name, layer)
            for B, F in ROUTE1_FRAMES:
                Lin = F * hop - (0 if B * F % 2 else 37) if layer == 0 else F * mult       # conv_in: a ragged T is the kernel's Lvalid
                add("route1", name, layer, 1, 1, 0, 0, B, Lin, "normal", enc_route1_class(name, layer, B, Lin))
            for kind in ("imp_first", "imp_last"):
                Lin = 3 * hop - 37 if layer == 0 else 3 * mult
                add("route1", name, layer, 1, 1, 0, 0, 2, Lin, kind, enc_route1_class(name, layer, 2, Lin))
    for layer in range(n_layers("full")):
        mult = frame_mult("full", layer)
        for B, F in ROUTE1_FULL:
            Lin = F * 320 - 37 if layer == 0 else F * mult
            add("route1", "full", layer, 1, 1, 0, 0, B, Lin, "normal", enc_route1_class("full", layer, B, Lin))
    return tuple(out)


def groups():
    """[(group, config, layer, route, variant)] in table order: one GPU test each, looping over its cases"""
    seen = []
    for c in cases():
        key = (c.group, c.config, c.layer, c.route, c.variant)
        if key not in seen:
            seen.append(key)
    return seen


def cases_of(key):
    return [c for c in cases() if (c.group, c.config, c.layer, c.route, c.variant) == tuple(key)]


def pcm_input(c):
    return c.layer == 0 or bool(c.flags & 4)


def input_keys():
    """the distinct (config, layer, pcm, B, Lin, kind) of the tables: what the references are computed for, once"""
    return sorted({(c.config, c.layer, pcm_input(c), c.B, c.Lin, c.kind) for c in cases()})


# ------------------------------------------------------------------------------------------------ inputs
def leaky(name, v):
    """LeakyReLU as every kernel and the oracle compute it: max(v, slope v) in f32"""
    slope = np.float32(config(name)[0].leaky_slope)
    return np.maximum(v, slope * v)


def make_input(name, layer, pcm, B, Lin, kind):
    """x [B][Cin][Lin], or PCM [B][Lin].  signed: stretches of +0.0, -0.0 and negatives beside the seeded normals, where
    max(v, slope v) and an activation applied twice (or not at all) differ"""
    shape = (B, Lin) if pcm else (B, layer_of(name, layer)["cin"], Lin)
    if kind in ("imp_first", "imp_last"):
        x = np.zeros(shape, np.float32)
        if pcm:
            x[B - 1, 0 if kind == "imp_first" else Lin - 1] = 1.0
        else:
            x[(B - 1, shape[1] - 1, 0) if kind == "imp_first" else (B - 1, 0, Lin - 1)] = 1.0
        return x
    rng = np.random.default_rng(zlib.crc32(repr((name, layer, pcm, B, Lin)).encode()))
    x = rng.standard_normal(shape, dtype=np.float32)
    if pcm:
        x *= np.float32(0.1)
    if kind == "signed":
        # stretches along a row's flattened (channel, time) index, period 97: they fall at other times in every channel, and a row
        # of a few samples still has them
        v = x.reshape(B, -1) if not pcm else x.reshape(1, -1)
        t = np.arange(v.shape[1]) % 97
        v[:, (t >= 5) & (t < 12)] = 0.0
        v[:, (t >= 20) & (t < 27)] = -0.0
        neg = (t >= 40) & (t < 60)
        v[:, neg] = -np.abs(v[:, neg])
    return x


def macs(name, layer, pcm, B, Lin):
    cfg = config(name)[0]
    ly = layer_of(name, layer)
    if pcm:
        L = cdiv(Lin, cfg.hop) * cfg.hop
        m = B * L * cfg.k_in * cfg.channels[0]
        return m if layer == 0 else m + B * (L // ly["s"]) * ly["cin"] * ly["cout"] * ly["k"]
    return B * (Lin // ly["s"]) * ly["cin"] * ly["cout"] * ly["k"]


def seam_rows(c):
    """the batch rows beside the forced seam of a case (the row that holds the seam column and its neighbours)"""
    plan = dict(c.env).get("RCA_CONV_BALANCE_PLAN")
    ly = layer_of(c.config, c.layer)
    cols = c.Lin // ly["s"]
    p = plan_of(plan, ly, c.B, cols, c.kclass)
    if p is None:
        return []
    r = p[0] * 64 // cols
    return [v for v in (r - 1, r, r + 1) if 0 <= v < c.B]


def oracle_rows(name, layer, pcm, B, Lin, extra=()):
    """the batch rows the CPU oracle computes (rows of a layer do not interact): all of them while the case stays under ~0.1 GMAC,
    else the first two, the last two, the two in the middle and `extra` (the rows beside a forced seam)"""
    if B <= 6 or macs(name, layer, pcm, B, Lin) <= GMAC_ALL_ROWS:
        return list(range(B))
    return sorted({0, 1, B // 2 - 1, B // 2, B - 2, B - 1, *extra})


def extra_rows(name, layer, pcm, B, Lin):
    """the seam rows of every forced-plan case that shares this input"""
    rows = set()
    for c in cases():
        if (c.config, c.layer, pcm_input(c), c.B, c.Lin) == (name, layer, pcm, B, Lin):
            rows.update(seam_rows(c))
    return tuple(sorted(rows))


# ------------------------------------------------------------------------------------------------ references
def layer_weights(name, layer):
    ly = layer_of(name, layer)
    w = config(name)[1]
    return w[ly["name"] + ".weight"], w[ly["name"] + ".bias"]


@functools.lru_cache(maxsize=None)
def oracle_codec(name):
    from oracle.codec import OracleCodec
    return OracleCodec(*config(name))


def oracle_layer(name, layer, x, pre=None):
    """the C oracle's conv1d of this layer on x [B][Cin][Lin]"""
    from oracle import codec as oc
    ly, (w, b) = layer_of(name, layer), layer_weights(name, layer)
    return oc.conv1d(x, w, b, ly["s"], ly["pre"] if pre is None else pre, config(name)[0].leaky_slope)


def oracle_pcm(name, layer, pcm):
    """layer 0 or 1 of the oracle's own encode pass on PCM rows (padded to whole frames by the oracle)"""
    return oracle_codec(name).encode(pcm, tap_layer=layer)[1]


def ref64(name, layer, x):
    """(y, m) in float64 and m = |b| + sum |w| |x|.  LeakyReLU is the model's f32 operation."""
    ly, (w, b) = layer_of(name, layer), layer_weights(name, layer)
    k, s = ly["k"], ly["s"]
    pad = (k - s + 1) // 2
    xa = x.astype(np.float32)
    if ly["pre"]:
        xa = leaky(name, xa)
    xa, w, b = xa.astype(np.float64), w.astype(np.float64), b.astype(np.float64)
    B, _, Lin = xa.shape
    Lout = Lin // s
    out = []
    for xv, wv, bv in ((xa, w, b), (np.abs(xa), np.abs(w), np.abs(b))):
        xp = np.zeros((B, ly["cin"], Lin + k))
        xp[:, :, pad:pad + Lin] = xv
        y = np.zeros((B, ly["cout"], Lout))
        for kk in range(k):
            y += np.matmul(wv[:, :, kk], xp[:, :, kk:kk + (Lout - 1) * s + 1:s])
        out.append(y + bv[None, :, None])
    return out[0], out[1]


def fma_bound(ly, m):
    return (ly["cin"] * ly["k"] + 1) * U * m


@functools.lru_cache(maxsize=24)
def reference(name, layer, pcm, B, Lin, kind):
    """(x, rows, want): the input, the rows the oracle ran on and its output [len(rows)][Cout][Lout] WITHOUT the activated store.
    Computed once per input and shared, read-only, by the flags, variants, plans and routes that use it."""
    x = make_input(name, layer, pcm, B, Lin, kind)
    rows = oracle_rows(name, layer, pcm, B, Lin, extra_rows(name, layer, pcm, B, Lin))
    xr = x if len(rows) == B else x[rows]
    want = oracle_pcm(name, layer, xr) if pcm else oracle_layer(name, layer, xr)
    x.setflags(write=False)
    want.setflags(write=False)
    return x, rows, want


def tap_input(c, x):
    """what the tap is fed: flag 1 hands it LeakyReLU(x), computed in f32 as the producing kernel would"""
    return leaky(c.config, x) if c.flags & 1 else x


def post_expected(c):
    """flag 2 asks for the activated store; the launch reports whether it made it (the consumer must be told).  Only the matrix
    kernel of the default variant can: s3's k6s3 layer runs the scalar chain in front of a layer that would take the hand-off"""
    return bool(c.flags & 2) and mfma_ok(layer_of(c.config, c.layer), c.variant)


def expected(c, want):
    """what the tap must return for the oracle's `want`: LeakyReLU(y) where the activated store is made; a view keeps the trailing columns"""
    y = leaky(c.config, want) if post_expected(c) else want
    return y[:, :, -c.view:] if c.view else y


def view_reference(c, x):
    """the whole view, halo columns included: the layer on the row cut at the view's left edge (zeros where the full launch reads
    samples), which is what a view computes"""
    ly = layer_of(c.config, c.layer)
    y = oracle_layer(c.config, c.layer, np.ascontiguousarray(x[:, :, x.shape[2] - c.view * ly["s"]:]))
    return leaky(c.config, y) if post_expected(c) else y


def first_mismatch(got, want):
    """'' when equal bit for bit as values (array_equal), else where and what the first difference is"""
    if np.array_equal(got, want):
        return ""
    bad = np.argwhere(~(got == want))
    b, co, t = (int(v) for v in bad[0])
    return f"{len(bad)} of {got.size} differ, first at (row {b}, channel {co}, position {t}): got {got[b, co, t]!r}, want {want[b, co, t]!r}"
