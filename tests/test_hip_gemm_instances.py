"""Every compiled gather-GEMM instance and schedule against the float64 oracle (-m gpu), and the ledger that records which
test runs each instance of csrc/ (CPU: test_instance_ledger_matches_csrc).

The tile variant, the loader form, the stage path (register ring / direct-to-LDS / deep ring), the schedule (one workgroup per
tile, stream-K, split-K) and the stream-K unit order are speed choices only: every one computes the same k-ordered fp32 fma
chains.  So each forced choice must (a) meet the float64 bar of test_conv_family_fuzz and (b) give the bits of the heuristic's
choice on the same plan and input (torch.equal) -- the invariant ops.import_tuning and bench.py's tuning file rely on.

How each instance is reached (csrc/conv_plan.hip, schedule() resolves a launch to one row of csrc/gather_gemm.hip's instance table):
  * vector loader, no prologue: Cin % 16 == 0, SNTC_PRO_NONE, register staging (dma=False or the default);
  * vector loader with prologue: Cin % 16 == 0, SNTC_PRO_ABS / SNTC_PRO_SQUARE;
  * dword gather (always with the prologue template argument): Cin % 16 != 0, any prologue;
  * direct-to-LDS (DMA): dma=True on a vector plan without prologue, variants 1..5, 8, 9; variants 6, 7, 10 have no such
    instance and fall back to register staging (same bits);
  * deep ring: variant 8, vector, no prologue, a static launch of at most two workgroups per CU, stage path not forced off
    (schedule()'s deep rule) -- every small forced-variant-8 launch below; dma=False turns it off;
  * COLM: stream-K on variant 9, vector, no prologue, register staging, one phase group, colm=True;
  * FUSE2: ConvPlan.fused (3x3 96 -> 96 + 1x1 96 -> 192);
  * bf16 x 3: bf16x3=True plans, variants 2 and 4 only (any other forced variant has no instance: SntcError).
"""
import ctypes as C
import hashlib
import json
import re
import zlib
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import ops_np as O

gpu = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "shallow-ntc_amd" / "csrc"
TOL = 2e-5          # the bar of test_conv_family_fuzz: |got - ref| <= TOL * max(|ref|, 1)
VARIANTS = range(1, 11)
DMA_VARIANTS = (1, 2, 3, 4, 5, 8, 9)
REF = {"conv": O.conv2d, "convT": O.conv2d_transpose, "sigdown": O.signal_conv_down, "sigup": O.signal_conv_up}
# epilogue formulas of include/sntc.h, v = act(conv + bias)
EPILOGUES = {
    0: lambda v, r, a: v,
    1: lambda v, r, a: v + r,
    2: lambda v, r, a: r + a * v,
    3: lambda v, r, a: r / v,
    4: lambda v, r, a: r * v,
    5: lambda v, r, a: r / np.sqrt(v),
    6: lambda v, r, a: r * np.sqrt(v),
    7: lambda v, r, a: np.where(r > 0, v, 0.0),
    8: lambda v, r, a: np.where(r >= 0, v, 0.2 * v),
}
PROLOGUES = {0: lambda x: x, 1: np.abs, 2: np.square}


# ---- the ledger: every compiled instance -> the test(s) that run it ---------------------------------------------------------
# Keys are the template argument lists as csrc/ spells them (whitespace removed); test_instance_ledger_matches_csrc fails when an
# instance exists that is not listed here, or a listed one no longer exists.
def _gg(tm, tn, wm, wn, *rest):
    return "gg_kernel<" + ",".join(str(v) for v in (tm, tn, wm, wn) + rest) + ">"


_SHAPES = [(1, 1, 4, 1), (1, 2, 4, 1), (1, 3, 4, 1), (1, 4, 4, 1), (1, 5, 4, 1), (1, 6, 4, 1), (1, 7, 4, 1), (1, 1, 2, 2),
           (2, 2, 2, 2), (2, 4, 4, 1)]
_DMA_SHAPES = [s for v, s in enumerate(_SHAPES, 1) if v in DMA_VARIANTS]
_ALL = "test_every_variant_on_ragged_shapes, test_every_variant_and_schedule_on_a_stream_k_launch, test_split_k_every_variant"
LEDGER = {}
for _s in _SHAPES:
    LEDGER[_gg(*_s, "true", "false")] = _ALL + ", test_epilogues_every_variant_and_schedule"
    LEDGER[_gg(*_s, "true", "true")] = "test_prologue_forms_every_variant, test_every_variant_and_schedule_on_a_stream_k_launch"
    LEDGER[_gg(*_s, "false", "true")] = _ALL + ", test_prologue_forms_every_variant"
for _s in _DMA_SHAPES:
    LEDGER[_gg(*_s, "true", "false", "false", "true")] = ("test_every_variant_on_ragged_shapes (dma=True), "
                                                          "test_every_variant_and_schedule_on_a_stream_k_launch (dma=True)")
LEDGER.update({
    _gg(1, 1, 2, 2, "true", "false", "false", "true", "kDeepRing"): "test_every_variant_on_ragged_shapes (variant 8, small launch)",
    _gg(1, 3, 4, 1, "true", "false", "false", "false", 0, "true"): "test_fused_tail_instance",
    _gg(2, 2, 2, 2, "true", "false", "false", "false", 0, "false", "true"): "test_every_variant_and_schedule_on_a_stream_k_launch (colm)",
    _gg(1, 2, 4, 1, "true", "false", "true"): "test_bf16x3_instances",
    _gg(1, 4, 4, 1, "true", "false", "true"): "test_bf16x3_instances",
    # launch switches of the small kernels: (source file, switch) -> case label
    "gdn_small<4>": "test_hip_ops.py::test_gdn_small_every_channel_count",
    "gdn_small<8>": "test_hip_ops.py::test_gdn_small_every_channel_count",
    "gdn_small<12>": "test_hip_ops.py::test_gdn_small_every_channel_count",
    "gdn_small<16>": "test_hip_ops.py::test_gdn_small_every_channel_count",
    "gdn_small<24>": "test_hip_ops.py::test_gdn_small_every_channel_count",
    "gdn_small<32>": "test_hip_ops.py::test_gdn_small_every_channel_count",
    "gdn_small<48>": "test_hip_ops.py::test_gdn_small_every_channel_count",
    "two_layer_tail<12>": "test_hip_ops.py::test_two_layer_tail_every_activation",
    "two_layer_tail<24>": "test_hip_ops.py::test_two_layer_tail_every_activation",
    "two_layer_tail<48>": "test_hip_ops.py::test_two_layer_tail_every_activation",
    "ssim_scale<1>": "test_hip_ops.py::test_image_quality_one_channel",
    "ssim_scale<3>": "test_hip_ops.py::test_ms_ssim",
    "rgb_conv<128>": "test_hip_ops.py::test_rgb_conv_every_instance",
    "rgb_conv<192>": "test_hip_ops.py::test_rgb_conv_every_instance",
    "rgb_conv<default>": "test_hip_ops.py::test_rgb_conv_every_instance",
    "wgrad<32>": "test_hip_train.py::test_conv_wgrad_gather_side_every_tile_width",
    "wgrad<64>": "test_hip_train.py::test_conv_wgrad_gather_side_every_tile_width",
    "wgrad<96>": "test_hip_train.py::test_conv_wgrad_gather_side_every_tile_width",
    "wgrad<128>": "test_hip_train.py::test_conv_wgrad_gather_side_every_tile_width",
    "wgrad<160>": "test_hip_train.py::test_conv_wgrad_gather_side_every_tile_width",
    "wgrad<default>": "test_hip_train.py::test_conv_wgrad_gather_side_every_tile_width",
    "colsum<true>": "test_hip_train.py::test_conv_wgrad_and_bias_grad",
    "colsum<false>": "test_hip_train.py::test_conv_wgrad_gather_side_every_tile_width",
    # the ten instances of the rANS coder (csrc/rans_kernel.h): element source x direction x table placement / symbol search
    "rans_encode<true>": "test_hip_bitstream.py::test_stream_words_match_python_restatement, "
                         "test_hip_bitstream.py::test_table_set_beyond_the_lds_limit",
    "rans_encode<false>": "test_hip_bitstream.py::test_table_set_beyond_the_lds_limit",
    "rans_decode<true>": "test_hip_bitstream.py::test_table_set_beyond_the_lds_limit, "
                         "test_hip_bitstream.py::test_full_chunk_boundary_in_every_decoder",
    "rans_decode<false>": "test_hip_bitstream.py::test_table_set_beyond_the_lds_limit",
    "rans_decode_fast": "test_hip_bitstream.py::test_start_tables_do_not_change_a_decoded_value, "
                        "test_hip_bitstream.py::test_full_chunk_boundary_in_every_decoder",
    "rans_encode_channels<true>": "test_hip_factorized_bitstream.py::test_channel_coder_words_and_values",
    "rans_encode_channels<false>": "test_hip_factorized_bitstream.py::test_every_table_placement_decodes_the_same_values",
    "rans_decode_channels<true>": "test_hip_factorized_bitstream.py::test_every_table_placement_decodes_the_same_values, "
                                  "test_hip_factorized_bitstream.py::test_an_empty_stream_in_both_coders",
    "rans_decode_channels<false>": "test_hip_factorized_bitstream.py::test_every_table_placement_decodes_the_same_values",
    "rans_decode_channels_fast": "test_hip_factorized_bitstream.py::test_channel_coder_words_and_values, "
                                 "test_hip_factorized_bitstream.py::test_every_table_placement_decodes_the_same_values",
})


def _strip(s):
    return re.sub(r"\s+", "", s)


def _compiled_gg_instances():
    """The gg_kernel<...> instantiations of csrc/gg_inst_*.hip: the INST macro bodies expanded over the shape list they are
    applied to (gather_gemm_kernel.h), plus the explicit lines."""
    hdr = (CSRC / "gather_gemm_kernel.h").read_text()
    lists = {}
    for name in ("SNTC_GG_SHAPES", "SNTC_GG_DMA_SHAPES"):
        m = re.search(r"#define\s+" + name + r"\s*\(\s*X\s*\)(.*)", hdr)
        assert m, name
        lists[name] = [tuple(int(v) for v in t.split(",")) for t in re.findall(r"X\s*\(([^)]*)\)", _strip(m.group(1)))]
    out = set()
    for path in sorted(CSRC.glob("gg_inst_*.hip")):
        text = path.read_text().replace("\\\n", " ")
        for line in text.splitlines():
            m = re.match(r"\s*#define\s+INST\s*\(([^)]*)\)(.*)", line)
            if m:
                params = _strip(m.group(1)).split(",")
                bodies = re.findall(r"gg_kernel\s*<([^>]*)>", m.group(2))
                use = re.search(r"(SNTC_GG_\w*SHAPES)\s*\(\s*INST\s*\)", text)
                assert use, path.name
                for shape in lists[use.group(1)]:
                    env = dict(zip(params, map(str, shape)))
                    for b in bodies:
                        out.add("gg_kernel<" + ",".join(env.get(a, a) for a in _strip(b).split(",")) + ">")
            elif re.match(r"\s*template\s+__global__\s+void\s+gg_kernel", line):
                out.add("gg_kernel<" + _strip(re.search(r"gg_kernel\s*<([^>]*)>", line).group(1)) + ">")
    return out


def _switch_cases(fname, anchor, label):
    """`case N:` labels of the switch in csrc/<fname> whose body holds `anchor` -> {label<N>}, plus label<default> if present."""
    text = (CSRC / fname).read_text()
    at = text.index(anchor)
    sw = text.rindex("switch", 0, at)
    body = text[sw:text.index("\n  }", sw)]
    out = {f"{label}<{v}>" for v in re.findall(r"case\s+(\d+)\s*:", body)}
    if re.search(r"default\s*:[^\n]*(LAUNCH|launch)", body):       # a default that launches something (not an error return)
        out.add(f"{label}<default>")
    return out


def _rans_instances():
    """The rANS coder's kernels in csrc/rans.hip and csrc/rans_channels.hip, as launched: rans_launch(k<true>, k<false>, ...) is
    the table-placement dispatch (tables staged in LDS or read from global memory), the start-table decoders are launched
    directly.  Every coder kernel the two files define must be launched, in every instance: a `template <bool LDS>` one in both."""
    launched, defined = set(), set()
    for fname in ("rans.hip", "rans_channels.hip"):
        text = (CSRC / fname).read_text()
        for k in re.findall(r"rans_launch\(\s*(rans_\w+?)_kernel\s*<\s*true\s*>\s*,\s*\1_kernel\s*<\s*false\s*>", text):
            launched |= {f"{k}<true>", f"{k}<false>"}
        launched |= set(re.findall(r"hipLaunchKernelGGL\(\s*(rans_(?:en|de)code\w*?)_kernel\s*,", text))
        for tmpl, k in re.findall(r"(template\s*<\s*bool\s+LDS\s*>\s*)?__global__\s+void\s+(?:__launch_bounds__\(\d+\)\s+)?"
                                  r"(rans_(?:en|de)code\w*?)_kernel\s*\(", text):
            defined |= {f"{k}<true>", f"{k}<false>"} if tmpl else {k}
    assert launched == defined and len(defined) == 10, (sorted(launched ^ defined), len(defined))
    return launched


def compiled_instances():
    out = _compiled_gg_instances()
    out |= _switch_cases("pixel.hip", "launch_gdn<4>", "gdn_small")
    out |= _switch_cases("pixel.hip", "launch_tail<12>", "two_layer_tail")
    out |= _switch_cases("msssim.hip", "(ssim_scale_kernel<1>)", "ssim_scale")
    out |= _switch_cases("rgb_conv.hip", "RGB_LAUNCH(4)", "rgb_conv")
    out |= _switch_cases("wgrad.hip", "SNTC_WG_LAUNCH(1, 1)", "wgrad")
    out |= {f"colsum<{v}>" for v in re.findall(r"colsum_kernel\s*<\s*(true|false)\s*>", (CSRC / "wgrad.hip").read_text())}
    out |= _rans_instances()
    return out


def test_instance_ledger_matches_csrc():
    """CPU: every compiled instance has a ledger entry naming the test that runs it, and every entry still exists."""
    have = compiled_instances()
    assert any(k.startswith("gg_kernel") for k in have), "the parser found no gather-GEMM instance"
    missing = sorted(have - set(LEDGER))
    stale = sorted(set(LEDGER) - have)
    assert not missing, f"compiled instances that no test is recorded to run: {missing}"
    assert not stale, f"ledger entries with no instance behind them: {stale}"
    for key, where in LEDGER.items():            # every test a ledger entry names exists
        refs = re.findall(r"(?:(\w+\.py)::)?(test_\w+)", where)
        assert refs, (key, where)
        for module, name in refs:
            src = (Path(__file__).parent / module if module else Path(__file__)).read_text()
            assert re.search(r"^def " + name + r"\(", src, re.M), (key, name)


# ---- helpers ----------------------------------------------------------------------------------------------------------------
def _dev_t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)


def _within(got, ref):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    assert got.shape == ref.shape
    err = np.abs(got.astype(np.float64) - ref).max()
    assert err <= TOL * max(np.abs(ref).max(), 1.0), err


def _layer(kind, k, cin, cout, seed, positive=False):
    rng = np.random.default_rng(seed)
    wshape = (k, k, cout, cin) if kind == "convT" else (k, k, cin, cout)
    if positive:        # GDN-like pools: v = conv + bias stays >= 1 for the division / square-root epilogues
        return rng, rng.uniform(0, 0.1, wshape).astype(np.float32), (1.0 + rng.random(cout)).astype(np.float32)
    return rng, (rng.standard_normal(wshape) / np.sqrt(max(k * k * cin / 4, 1))).astype(np.float32), rng.standard_normal(cout).astype(np.float32)


class _state:
    """Restores the process-wide schedule state and leaves the stream-K status word clear (tests/test_hip_fullsize.py)."""

    def __init__(self, *plans):
        self.plans = plans

    def __enter__(self):
        from shallow_ntc_amd import ops
        self.sk = ops.stream_k_enabled()
        ops.set_stream_k(True)
        return self

    def __exit__(self, *exc):
        from shallow_ntc_amd import ops
        try:
            for p in self.plans:
                p.set_tile(0)
                p.set_stream_k(True)
                p.clear_tuning()
        finally:
            try:
                ops.set_stream_k(self.sk)
            finally:
                if exc[0] is not None:
                    ops.take_conv_status()      # a test that failed part-way leaves the word clear, not flagged for the next test
        if exc[0] is None:
            ops.check_conv_status()             # no stream-K hand-off of this test timed out
        return False


def _ws_bytes(plan, n, h, w):
    from shallow_ntc_amd import _capi as capi
    return int(capi.load().sntc_conv_workspace_bytes(plan._h, n, h, w))


def _order(plan, n, h, w):
    from shallow_ntc_amd import _capi as capi
    o = C.c_int(-1)
    capi.call("sntc_conv_launch_order", plan._h, n, h, w, C.byref(o))
    return o.value


# ---- shapes where kernels go wrong: M, N and K ragged at once ---------------------------------------------------------------
RAGGED = [  # kind, k, s, cin, cout, n, h, w, act
    ("conv", 1, 1, 33, 40, 3, 7, 9, "relu"),           # gather, K = 33
    ("conv", 1, 1, 48, 200, 3, 5, 7, None),            # vector, N = 200
    ("conv", 3, 1, 12, 5, 3, 5, 7, "leaky_relu"),      # gather, K = 108
    ("conv", 3, 1, 32, 100, 1, 13, 11, None),
    ("conv", 5, 2, 3, 100, 2, 9, 11, "sigmoid"),       # the RGB layer's K = 75
    ("conv", 5, 2, 48, 1, 3, 7, 5, None),              # one output channel
    ("convT", 5, 2, 33, 40, 1, 1, 1, None),            # one-pixel image, four phase groups of K 297 / 198 / 198 / 132
    ("convT", 5, 2, 64, 200, 3, 5, 7, "relu"),
    ("convT", 13, 8, 16, 5, 3, 3, 2, None),
    ("sigdown", 5, 2, 12, 100, 2, 9, 7, None),
    ("sigup", 5, 2, 32, 1, 3, 3, 5, None),
    ("sigup", 3, 1, 33, 40, 1, 1, 1, "relu"),
]


def _ragged_case(case, dev):
    from shallow_ntc_amd import ops
    kind, k, s, cin, cout, n, h, w, act = case
    rng, wk, b = _layer(kind, k, cin, cout, zlib.crc32(repr(case).encode()))
    x = rng.standard_normal((n, h, w, cin)).astype(np.float32)
    ref = O.ACTIVATIONS[act](REF[kind](x, wk, b, s))
    plan = ops.ConvPlan(kind, _dev_t(wk, dev), _dev_t(b, dev), s, act)
    return plan, _dev_t(x, dev), ref


@gpu
@pytest.mark.parametrize("case", RAGGED, ids=lambda c: "-".join(map(str, c)))
def test_every_variant_on_ragged_shapes(case, dev):
    """Variants 1..10 forced, each on the register ring and with direct-to-LDS staging asked for (variants without a DMA instance
    fall back to the register ring; variant 8 at these sizes runs the deep ring unless dma=False), the static schedule; then every
    candidate of the tuning machinery through set_choice.  All of them: the float64 bar and the heuristic's bits."""
    kind, k, s, cin, cout, n, h, w, act = case
    plan, x, ref = _ragged_case(case, dev)
    with _state(plan):
        y0 = plan(x).clone()
        _within(y0, ref)
        for v in VARIANTS:
            plan.set_tile(v)
            assert plan.launch_info(n, h, w)[0] == v
            for dma in (None, True, False):
                plan.set_stream_k(False, dma=dma)
                y = plan(x)
                _within(y, ref)
                assert torch.equal(y, y0), (v, dma)
        plan.set_tile(0)
        plan.set_stream_k(True)
        cands = plan.candidates(n, h, w)
        assert cands and all(1 <= v <= 10 for v, _ in cands)
        for v, sk in cands:
            plan.set_choice(n, h, w, v, sk)
            assert plan.launch_info(n, h, w)[0] == v
            assert torch.equal(plan(x), y0), (v, sk)


# ---- prologue forms (GDN norm pools): vector + prologue and gather + prologue ------------------------------------------------
PRO_CASES = [  # cin (= cout), prologue, epilogue, n, h, w
    (48, 1, 3, 3, 7, 9),     # |x| -> res / v            (GDN1)
    (48, 2, 5, 1, 13, 11),   # x^2 -> res / sqrt(v)      (classic GDN)
    (33, 1, 4, 3, 5, 7),     # gather: |x| -> res * v    (inverse GDN1)
    (12, 2, 6, 2, 9, 7),     # gather: x^2 -> res * sqrt(v)
]


@gpu
@pytest.mark.parametrize("case", PRO_CASES, ids=lambda c: "-".join(map(str, c)))
def test_prologue_forms_every_variant(case, dev):
    from shallow_ntc_amd import ops
    c, pro, epi, n, h, w = case
    rng, wk, b = _layer("conv", 1, c, c, zlib.crc32(repr(case).encode()), positive=True)
    x = rng.standard_normal((n, h, w, c)).astype(np.float32)
    ref = EPILOGUES[epi](O.conv2d(PROLOGUES[pro](x.astype(np.float64)), wk, b, 1), x.astype(np.float64), None)
    plan = ops.ConvPlan("conv", _dev_t(wk, dev), _dev_t(b, dev), 1, None, pro, epi)
    xd = _dev_t(x, dev)
    with _state(plan):
        y0 = plan(xd, res=xd).clone()
        _within(y0, ref)
        for v in VARIANTS:
            plan.set_tile(v)
            for dma in (None, True):           # direct-to-LDS has no prologue form: asking for it keeps the register ring
                plan.set_stream_k(False, dma=dma)
                assert plan.launch_info(n, h, w)[0] == v
                y = plan(xd, res=xd)
                _within(y, ref)
                assert torch.equal(y, y0), (v, dma)


# ---- stream-K: a launch large enough that every variant's workers all get work ----------------------------------------------
SK_CASES = [  # cin, cout, prologue, epilogue     (1x1, n = 2, 271 x 263: M = 142546, ragged for every tile height; more tiles
              # than resident workers for every variant, 256 x 128 included, so that workers really hand tiles on)
    (48, 100, 0, 0),
    (33, 100, 0, 0),
    (48, 48, 2, 5),
    (33, 33, 1, 3),
]
SK_N, SK_H, SK_W = 2, 271, 263
# SHA-256 of the heuristic's float32 output bytes per case, recorded with the library of the commit before the piece walk moved to
# csrc/gg_pieces.h: every instance below is torch.equal to that output, so one comparison pins them all to those bits
SK_DIGESTS = json.loads((ROOT / "tests" / "golden" / "gg_pieces_digests.json").read_text())["fp32_sk_cases"]


@gpu
@pytest.mark.parametrize("case", SK_CASES, ids=lambda c: "-".join(map(str, c)))
def test_every_variant_and_schedule_on_a_stream_k_launch(case, dev):
    """Each variant forced under the static schedule and forced stream-K (the launch really is cut: fewer workgroups), each with
    the register ring and direct-to-LDS staging asked for; on variant 9 both stream-K unit orders (the COLM twin where it exists,
    the strip-major fallback where it does not); every candidate through set_choice."""
    from shallow_ntc_amd import ops
    cin, cout, pro, epi = case
    n, h, w = SK_N, SK_H, SK_W
    gdn = pro != 0
    rng, wk, b = _layer("conv", 1, cin, cout, zlib.crc32(repr(case).encode()), positive=gdn)
    x = rng.standard_normal((n, h, w, cin)).astype(np.float32)
    ref = EPILOGUES[epi](O.conv2d(PROLOGUES[pro](x.astype(np.float64)), wk, b, 1), x.astype(np.float64), None)
    plan = ops.ConvPlan("conv", _dev_t(wk, dev), _dev_t(b, dev), 1, None, pro, epi)
    xd = _dev_t(x, dev)
    res = xd if epi else None
    workers = {}
    with _state(plan):
        y0 = plan(xd, res=res).clone()
        got = hashlib.sha256(y0.cpu().numpy().tobytes()).hexdigest()
        print("DIGEST fp32_sk_cases", "-".join(map(str, case)), got)
        assert got == SK_DIGESTS.get("-".join(map(str, case))), (got, "recorded in tests/golden/gg_pieces_digests.json: re-record only "
                                                                      "with a deliberate change of the fp32 arithmetic")
        _within(y0, ref)
        for v in VARIANTS:
            plan.set_tile(v)
            for dma in (False, True):
                plan.set_stream_k(False, dma=dma)
                v_st, nb_static = plan.launch_info(n, h, w)
                assert v_st == v and torch.equal(plan(xd, res=res), y0), (v, "static", dma)
                plan.set_stream_k(True, dma=dma, force=True, colm=False)
                v_sk, nb_sk = plan.launch_info(n, h, w)
                assert v_sk == v and nb_sk < nb_static, (v, nb_sk, nb_static)       # the persistent workers really run it ...
                workers[v, dma] = nb_sk
                assert _ws_bytes(plan, n, h, w) > 0, v                              # ... with their hand-off scratch
                assert _order(plan, n, h, w) == 0
                assert torch.equal(plan(xd, res=res), y0), (v, "stream-K", dma)
                plan.set_stream_k(True, dma=dma, force=True, colm=True)
                colm = v == 9 and cin % 16 == 0 and not gdn and not dma
                assert _order(plan, n, h, w) == int(colm), (v, dma)                   # the twin only where it exists
                assert torch.equal(plan(xd, res=res), y0), (v, "colm", dma)
            ops.check_conv_status()
        # which stage path ran shows in the stream-K worker count: one per resident workgroup of the instance launched.  Where
        # no direct-to-LDS instance exists (variants 6, 7, 10; the gather and prologue forms) asking for one must give the
        # register ring's residency -- the documented fallback; where one exists, its larger ring changes the residency
        dma_path = cin % 16 == 0 and not gdn
        for v in VARIANTS:
            if not dma_path or v not in DMA_VARIANTS:
                assert workers[v, True] == workers[v, False], (v, workers[v, True], workers[v, False])
        if dma_path:
            assert any(workers[v, True] != workers[v, False] for v in DMA_VARIANTS), workers
        plan.set_tile(0)
        plan.set_stream_k(True)
        cands = plan.candidates(n, h, w)
        assert any(sk for _, sk in cands), cands
        for v, sk in cands:
            plan.set_choice(n, h, w, v, sk)
            assert torch.equal(plan(xd, res=res), y0), (v, sk)


# ---- every epilogue, two variants, static and stream-K, at a ragged shape ---------------------------------------------------
@gpu
@pytest.mark.parametrize("epi", range(9))
def test_epilogues_every_variant_and_schedule(epi, dev):
    from shallow_ntc_amd import ops
    cin, cout = 48, 40
    n, h, w = SK_N, SK_H, SK_W
    rng, wk, b = _layer("conv", 1, cin, cout, 100 + epi, positive=True)
    x = rng.random((n, h, w, cin)).astype(np.float32)
    r = rng.standard_normal((n, h, w, cout)).astype(np.float32)
    r[0, 0, 0, :4] = 0.0                          # the masks' boundary (relu: > 0, leaky: >= 0)
    a = rng.standard_normal((n, h, w, cout)).astype(np.float32)
    act = "relu" if epi in (1, 2) else None
    v64 = O.ACTIVATIONS[act](O.conv2d(x, wk, b, 1))
    ref = EPILOGUES[epi](v64, r.astype(np.float64), a.astype(np.float64))
    plan = ops.ConvPlan("conv", _dev_t(wk, dev), _dev_t(b, dev), 1, act, 0, epi)
    xd, rd, ad = _dev_t(x, dev), _dev_t(r, dev), _dev_t(a, dev)
    with _state(plan):
        y0 = plan(xd, res=rd, aux=ad).clone()
        _within(y0, ref)
        for v in (2, 9):
            plan.set_tile(v)
            for sk in (False, True):
                plan.set_stream_k(sk, force=sk)
                y = plan(xd, res=rd, aux=ad)
                _within(y, ref)
                assert torch.equal(y, y0), (v, sk)


# ---- split-K: few tiles per image, a long contraction -----------------------------------------------------------------------
SPLIT_CASES = [  # kind, k, s, cin, cout, n, h, w
    ("conv", 3, 1, 256, 100, 3, 9, 7),          # vector, K = 2304
    ("sigdown", 9, 4, 33, 40, 3, 17, 13),       # gather, K = 2673
    ("convT", 5, 2, 400, 5, 3, 3, 5),           # four phase groups, 50 ... 112 stages of 32
]


@gpu
@pytest.mark.parametrize("case", SPLIT_CASES, ids=lambda c: "-".join(map(str, c)))
def test_split_k_every_variant(case, dev):
    """pick_ksplit > 1 (its comment: the split depends on the layer and the per-image geometry only, so image i alone is bit-identical
    to image i inside the batch) -- for every forced variant."""
    from shallow_ntc_amd import ops
    kind, k, s, cin, cout, n, h, w = case
    rng, wk, b = _layer(kind, k, cin, cout, zlib.crc32(repr(case).encode()))
    x = rng.standard_normal((n, h, w, cin)).astype(np.float32)
    ref = REF[kind](x, wk, b, s)
    plan = ops.ConvPlan(kind, _dev_t(wk, dev), _dev_t(b, dev), s)
    xd = _dev_t(x, dev)
    with _state(plan):
        y0 = plan(xd).clone()
        _within(y0, ref)
        for v in VARIANTS:
            plan.set_tile(v)
            for dma in (False, True):
                plan.set_stream_k(False, dma=dma)
                assert _ws_bytes(plan, n, h, w) > 0, v          # the split-K slabs: this shape does take the split path
                y = plan(xd)
                _within(y, ref)
                assert torch.equal(y, y0), (v, dma)
                for i in range(n):
                    assert torch.equal(plan(xd[i:i + 1].contiguous()), y0[i:i + 1]), (v, dma, i)


# ---- the channel pairs the committed tuning file pins, with the variants it pins for them ------------------------------------
def _tuned_pairs():
    entries = json.loads((ROOT / "profiles" / "tuning_gfx950.json").read_text())["entries"]
    pins = {}
    for _idx, kind, cin, cout, _n, _h, _w, v, _sk in entries:
        pins.setdefault((kind, cin, cout), set()).add(int(v))
    return sorted((kind, cin, cout, tuple(sorted(vs))) for (kind, cin, cout), vs in pins.items())


@gpu
@pytest.mark.parametrize("pair", _tuned_pairs(), ids=lambda p: "-".join(map(str, p[:3])))
def test_tuning_file_pairs_with_their_pinned_variants(pair, dev):
    """Reduced spatial size (the stream-K form of each pinned variant is the same instance, tested above at full size)."""
    from shallow_ntc_amd import ops
    kind, cin, cout, pinned = pair
    for k, s, n, h, w in ((3, 1, 1, 5, 7), (5, 2, 2, 5, 3) if kind == "convT" else (5, 2, 2, 9, 7)):
        rng, wk, b = _layer(kind, k, cin, cout, zlib.crc32(repr((pair, k)).encode()))
        x = rng.standard_normal((n, h, w, cin)).astype(np.float32)
        ref = O.relu(REF[kind](x, wk, b, s))
        plan = ops.ConvPlan(kind, _dev_t(wk, dev), _dev_t(b, dev), s, "relu")
        xd = _dev_t(x, dev)
        with _state(plan):
            y0 = plan(xd).clone()
            _within(y0, ref)
            for v in pinned:
                plan.set_tile(v)
                assert plan.launch_info(n, h, w)[0] == v
                y = plan(xd)
                _within(y, ref)
                assert torch.equal(y, y0), (k, v)


# ---- FUSE2, bf16 x 3 -----------------------------------------------------------------------------------------------------
@gpu
def test_fused_tail_instance(dev):
    """The 128 x 96 fused ResidualBlock tail instance at a ragged row count, skip epilogue: float64 and the two launches' bits."""
    from shallow_ntc_amd import _capi as capi
    from shallow_ntc_amd import ops
    n, h, w = 3, 5, 7
    rng, w1, b1 = _layer("conv", 3, 96, 96, 91)
    _, w2, b2 = _layer("conv", 1, 96, 192, 92)
    x = rng.standard_normal((n, h, w, 96)).astype(np.float32)
    r = rng.standard_normal((n, h, w, 192)).astype(np.float32)
    ref = O.conv2d(O.relu(O.conv2d(x, w1, b1, 1)), w2, b2, 1) + r
    first = ops.ConvPlan("conv", _dev_t(w1, dev), _dev_t(b1, dev), 1, "relu")
    second = ops.ConvPlan("conv", _dev_t(w2, dev), _dev_t(b2, dev), 1, None, capi.PRO_NONE, capi.EPI_ADD)
    assert first.fusable_with(second)
    xd, rd = _dev_t(x, dev), _dev_t(r, dev)
    one = first.fused(second, xd, res=rd)
    _within(one, ref)
    assert torch.equal(one, second(first(xd), res=rd))


@gpu
def test_bf16x3_instances(dev):
    """bf16 x 3 plans: variants 2 and 4 at a ragged shape against float64; every other forced variant has no instance and the call
    fails loudly instead of running something else."""
    from shallow_ntc_amd import _capi as capi
    from shallow_ntc_amd import ops
    n, h, w = 3, 5, 7
    rng, wk, b = _layer("convT", 5, 32, 40, 93)
    x = rng.standard_normal((n, h, w, 32)).astype(np.float32)
    ref = O.conv2d_transpose(x, wk, b, 2)
    plan = ops.ConvPlan("convT", _dev_t(wk, dev), _dev_t(b, dev), 2, bf16x3=True)
    xd = _dev_t(x, dev)
    with _state(plan):
        _within(plan(xd), ref)
        for v in VARIANTS:
            plan.set_tile(v)
            plan.set_stream_k(False)
            if v in (2, 4):
                _within(plan(xd), ref)
            else:
                with pytest.raises(capi.SntcError):
                    plan(xd)
