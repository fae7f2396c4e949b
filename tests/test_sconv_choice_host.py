"""Host test of the launch of a sparse convolution (sconv_choose, egonn_amd/csrc/sconv.hip) through egonn_debug_sconv_choice,
which makes no device call: route, kernel template and template parameters, grid, block and dynamic LDS bytes of a layer under a
setting, for the product rule on every layer of the EgoNN trunk and head, on both sides of every threshold of the rule, for every
debug code and for the combinations the launchers refuse.  The expected values are literals: kernel, template arguments, grid and
block are read off the kernel trace of the parent of the change that introduced sconv_choose
(profiles/sconv_choice_trace.txt: the smoke batch, whose maps hold 576 / 352 / 224 / 112 / 64 / 48 / 48 row groups on
levels 1-7), the others and the LDS bytes are worked out by hand from the rule as DESIGN.md states it ("Host side of a
convolution") — none is computed by a copy of the rule.  tests/test_gpu_launch_tags.py sees only the family name; a moved
threshold or a swapped template argument shows here.  Runs with the EGONN_* measurement switches unset."""
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = ("EGONN_SPLIT_CFG", "EGONN_SPLIT_MAX_LEVEL", "EGONN_SPLIT_MAX_LEVEL_K8", "EGONN_NO_TAIL_SPLIT", "EGONN_KSPLIT", "EGONN_KSPLIT8",
            "EGONN_KSPLIT_KW", "EGONN_KSPLIT_KW8", "EGONN_KSPLIT_PARTS")


@pytest.fixture(scope="module")
def choice():
    for s in SWITCHES:
        assert s not in os.environ, "the expected choices are those of the product rule"
    import __graft_entry__ as g
    g.build()
    from egonn_amd import _lib
    return _lib.debug_sconv_choice


def _full(route, kernel, grid, block, lds, **tp):
    d = dict(route=route, kernel=kernel, NW=0, NSW=0, KW=0, KS=0, GATED=0, TRACE=0, resident=0, KSP=0, D=0, G=0, SPLIT=0, PIPE=0,
             gx=grid[0], gy=grid[1], gz=grid[2], block=block, lds=lds, kparts=1)
    d.update(tp)
    return d


def SP(nw, nsw, kw, grid, block, lds, **tp):      # sconv_split_kernel<cin, cout, NW, NSW, TRACE, GATED, KS, KW>
    return _full("split", "split", grid, block, lds, NW=nw, NSW=nsw, KW=kw, **tp)


def RES(nw, gx, block, lds, **tp):                # sconv_split_resident_kernel<NW, GATED>
    return _full("split", "split", (gx, 1, 1), block, lds, NW=nw, resident=1, **tp)


def RG(ksp, d, g, gx, block, lds, route="rg", **tp):   # sconv_rg_kernel<cin, cout, BF16, D, KSP, G, NW = KSP, SPLIT>
    return _full(route, "rg", (gx, 1, 1), block, lds, NW=ksp, KSP=ksp, D=d, G=g, **tp)


def DMA(ksp, d, gx, block, lds, **tp):            # sconv_dma_kernel<cin, cout, D, KSP, NW = KSP, TRACE, PIPE>
    return _full("dma", "dma", (gx, 1, 1), block, lds, NW=ksp, KSP=ksp, D=d, **tp)


def WG(gx, lds):                                  # sconv_wg_kernel<cin, cout, BF16, 4>
    return _full("wg", "wg", (gx, 1, 1), 256, lds, NW=4)


GROUPS = {1: 576, 2: 352, 3: 224, 4: 112, 5: 64, 6: 48, 7: 48}     # of the smoke batch (the trace)
TAIL = RG(4, 6, 1, 192, 256, 24832, route="tail_split", SPLIT=1)
RG6 = RG(4, 6, 1, 192, 256, 24832)
KW2_64 = SP(4, 2, 2, (56, 1, 1), 512, 81920)
L5_KW2 = SP(4, 2, 2, (16, 2, 1), 512, 81920)
# the layers of the forward in launch order: (map kind, output level, cin, cout), then the launch under the fp32 product rule
# (gated: level 2's strided convolution reads level 1's block tail), exact fp32 (split level limit -1), bf16 maps, and fp32 with
# operand autoscale (no resident form, no tail split)
LAYERS = [
    ((1, 1, 32, 32), RES(8, 72, 512, 81920), DMA(1, 4, 576, 64, 10368, PIPE=1), RG(1, 4, 2, 288, 64, 4160), SP(4, 1, 1, (144, 1, 1), 256, 32768)),
    ((0, 1, 32, 32), SP(4, 1, 1, (144, 1, 1), 256, 32768), DMA(1, 4, 576, 64, 10368, PIPE=1), RG(1, 4, 2, 288, 64, 4160), SP(4, 1, 1, (144, 1, 1), 256, 32768)),
    ((1, 2, 32, 32), RES(12, 32, 768, 137216, GATED=1), DMA(1, 4, 352, 64, 10368, PIPE=1), RG(1, 4, 2, 176, 64, 4160), SP(4, 1, 1, (88, 1, 1), 256, 32768)),
    ((0, 2, 32, 64), SP(4, 1, 1, (88, 2, 1), 256, 32768), DMA(1, 4, 704, 64, 10368, PIPE=1), WG(88, 15360), SP(4, 1, 1, (88, 2, 1), 256, 32768)),
    ((0, 2, 64, 64), SP(4, 1, 1, (88, 2, 1), 256, 32768), DMA(2, 4, 704, 128, 20736, PIPE=1), WG(88, 15360), SP(4, 1, 1, (88, 2, 1), 256, 32768)),
    ((1, 3, 64, 64), KW2_64, DMA(2, 4, 448, 128, 20736, PIPE=1), WG(56, 15360), KW2_64),
    ((0, 3, 64, 64), KW2_64, DMA(2, 4, 448, 128, 20736, PIPE=1), WG(56, 15360), KW2_64),
    ((1, 4, 64, 64), SP(4, 2, 2, (32, 1, 1), 512, 81920), DMA(2, 4, 224, 128, 20736, PIPE=1), WG(32, 15360), SP(4, 2, 2, (32, 1, 1), 512, 81920)),
    ((0, 4, 64, 128), SP(4, 2, 2, (32, 2, 1), 512, 81920), DMA(2, 4, 448, 128, 20736, PIPE=1), WG(32, 23552), SP(4, 2, 2, (32, 2, 1), 512, 81920)),
    ((0, 4, 128, 128), SP(4, 2, 2, (32, 2, 1), 512, 81920), DMA(4, 4, 448, 256, 41472, PIPE=1), WG(32, 23552), SP(4, 2, 2, (32, 2, 1), 512, 81920)),
    ((1, 5, 128, 128), L5_KW2, RG(4, 6, 1, 256, 256, 24832), RG(4, 4, 2, 128, 256, 49408), L5_KW2),
    ((0, 5, 128, 128), L5_KW2, RG(4, 6, 1, 256, 256, 24832), RG(4, 4, 2, 128, 256, 49408), L5_KW2),
    ((1, 6, 128, 128), TAIL, RG6, RG6, RG6),
    ((0, 6, 128, 128), TAIL, RG6, RG6, RG6),
    ((1, 7, 128, 128), TAIL, RG6, RG6, RG6),
    ((0, 7, 128, 128), TAIL, RG6, RG6, RG6),
    ((2, 3, 64, 64), KW2_64, DMA(2, 4, 448, 128, 20736, PIPE=1), WG(56, 15360), KW2_64),
    ((2, 6, 128, 128), TAIL, RG6, RG6, RG6),
    ((2, 5, 128, 128), L5_KW2, RG(4, 6, 1, 256, 256, 24832), RG(4, 4, 2, 128, 256, 49408), L5_KW2),
]
PRECISIONS = {"fp32": dict(), "fp32_exact": dict(split_max_level=-1), "bf16": dict(bf16=1), "autoscale": dict(autoscale=1)}


@pytest.mark.parametrize("col,setting", list(enumerate(PRECISIONS, 1)), ids=list(PRECISIONS))
@pytest.mark.parametrize("row", LAYERS, ids=[f"kind{l[0][0]}-L{l[0][1]}-{l[0][2]}to{l[0][3]}" for l in LAYERS])
def test_product_rule_on_the_forward(choice, row, col, setting):
    kind, level, cin, cout = row[0]
    gated = setting == "fp32" and (kind, level) == (1, 2)
    assert choice(kind, level, cin, cout, GROUPS[level], gated=gated, **PRECISIONS[setting]) == row[col]


L3 = (0, 3, 64, 64, 224)       # a level-3 k=3 layer of the smoke batch
# (layer, settings) -> the launch
CASES = {
    # split level limit: level 5 / 6 under limits 5 and 6 (level 6 has no KW rule: two column parts below one round of the chip)
    "limit5-L5": (((0, 5, 128, 128, 64), dict()), L5_KW2),
    "limit5-L6": (((0, 6, 128, 128, 48), dict()), TAIL),
    "limit6-L6": (((0, 6, 128, 128, 48), dict(split_max_level=6)), SP(4, 2, 1, (16, 2, 1), 256, 40960)),
    "limit6-L7": (((0, 7, 128, 128, 48), dict(split_max_level=6)), TAIL),
    # the tail split is the 128->128 plan's and off under autoscale
    "tail-autoscale": (((0, 6, 128, 128, 48), dict(autoscale=1)), RG6),
    "tail-256": (((0, 6, 256, 256, 48), dict()), RG(4, 6, 1, 384, 256, 24832)),
    # column parts: two per task while ceil(groups / 4) < 700
    "parts-699": (((0, 2, 64, 64, 2796), dict()), SP(4, 1, 1, (704, 2, 1), 256, 32768)),
    "parts-700": (((0, 2, 64, 64, 2797), dict()), SP(4, 2, 1, (704, 1, 1), 256, 40960)),
    # bf16: four groups per wave from 32768 task slots (groups * cout/32 * KSP)
    "bf16-G4-32768": (((0, 1, 32, 32, 32768), dict(bf16=1)), RG(1, 3, 4, 8192, 64, 7232)),
    "bf16-G2-32767": (((0, 1, 32, 32, 32767), dict(bf16=1)), RG(1, 4, 2, 16384, 64, 4160)),
    "bf16-G4-64to64": (((0, 5, 64, 64, 8192), dict(bf16=1)), RG(2, 3, 4, 4096, 128, 47232)),
    # small: level 5 in fp32, level 6 in bf16 (the level below: the LDS-DMA kernel / two groups per wave)
    "small-fp32-L4": (((0, 4, 128, 128, 112), dict(split_max_level=-1)), DMA(4, 4, 448, 256, 41472, PIPE=1)),
    "small-fp32-L5": (((0, 5, 128, 128, 64), dict(split_max_level=-1)), RG(4, 6, 1, 256, 256, 24832)),
    "small-bf16-L5": (((0, 5, 128, 128, 64), dict(bf16=1)), RG(4, 4, 2, 128, 256, 49408)),
    "small-bf16-L6": (((0, 6, 128, 128, 48), dict(bf16=1)), RG6),
    # cooperative kernel: bf16, cin * cout >= 2048, level <= 4
    "coop-1024": (((0, 2, 32, 32, 352), dict(bf16=1)), RG(1, 4, 2, 176, 64, 4160)),
    "coop-2048": (((0, 2, 32, 64, 352), dict(bf16=1)), WG(88, 15360)),
    "coop-L4": (((0, 4, 128, 128, 112), dict(bf16=1)), WG(32, 23552)),
    "coop-L5": (((0, 5, 128, 128, 64), dict(bf16=1)), RG(4, 4, 2, 128, 256, 49408)),
    # resident grid: 512 workgroups on the 8-slot maps, 256 on k=3 and gated ones, clipped by the capacity, or the override
    "resident-512": (((1, 1, 32, 32, 100000), dict()), RES(8, 512, 512, 81920)),
    "resident-k3-256": (((0, 1, 32, 32, 100000), dict(resident_mask=7)), RES(8, 256, 512, 159744)),
    "resident-gated-256": (((1, 2, 32, 32, 100000), dict(gated=1)), RES(12, 256, 768, 137216, GATED=1)),
    "resident-clipped": (((1, 1, 32, 32, 4000), dict()), RES(8, 504, 512, 81920)),
    "resident-override": (((1, 1, 32, 32, 576), dict(max_workgroups=100)), RES(8, 100, 512, 81920)),
    "resident-mask-off": (((1, 1, 32, 32, 576), dict(resident_mask=0)), SP(4, 1, 1, (144, 1, 1), 256, 32768)),
    # offset parts: KW 2 on levels 3-5 forces 64 columns per workgroup; cin < 64 drops KW; a gated input drops kparts and KW
    "kw2-L2-none": (((0, 2, 64, 128, 352), dict()), SP(4, 2, 1, (88, 2, 1), 256, 40960)),
    "kw2-L3": (((0, 3, 64, 128, 224), dict()), SP(4, 2, 2, (56, 2, 1), 512, 81920)),
    "kw2-L5": (((0, 5, 64, 128, 64), dict()), SP(4, 2, 2, (16, 2, 1), 512, 81920)),
    "kw2-L6-none": (((0, 6, 64, 128, 48), dict(split_max_level=6)), SP(4, 2, 1, (16, 2, 1), 256, 40960)),
    "kw-cin32": (((0, 3, 32, 64, 224), dict()), SP(4, 1, 1, (56, 2, 1), 256, 32768)),
    "kw3-64-columns": (((0, 4, 128, 128, 112), dict(kw=3)), SP(4, 2, 3, (32, 2, 1), 768, 122880)),
    "kw4-one-slice": (((0, 4, 128, 128, 112), dict(kw=4, col_parts=4)), SP(4, 1, 4, (32, 4, 1), 1024, 131072)),
    "kw3-too-large": (((0, 4, 128, 128, 112), dict(kw=3, col_parts=1, kparts=2)), SP(4, 4, 1, (32, 1, 2), 256, 57344, KS=1, kparts=2)),
    "kparts2": (((0, 5, 128, 128, 64), dict(kparts=2)), SP(4, 2, 2, (16, 2, 2), 512, 81920, KS=1, kparts=2)),
    "gated-lockstep": (((1, 2, 32, 32, 352), dict(gated=1, resident_mask=0, kparts=2)), SP(4, 1, 1, (88, 1, 1), 256, 49152, GATED=1)),
    # every debug code (include/egonn_hip.h)
    "code1": ((L3, dict(code=1)), _full("plain", "plain", (0, 1, 1), 0, 0)),
    "code2": ((L3, dict(code=2)), RG(2, 3, 1, 448, 128, 12416)),
    "code4": ((L3, dict(code=4)), WG(56, 23552)),
    "code8": ((L3, dict(code=8)), RG(2, 3, 2, 224, 128, 24704)),
    "code8-small": (((0, 5, 128, 128, 64), dict(code=8)), RG(4, 6, 1, 256, 256, 24832)),
    "code16": ((L3, dict(code=16)), DMA(2, 4, 448, 128, 20736, PIPE=1)),
    "code16-L5": (((0, 5, 128, 128, 64), dict(code=16)), DMA(4, 4, 256, 256, 41472, PIPE=1)),
    "code16-bf16": ((L3, dict(code=16, bf16=1)), RG(2, 4, 1, 448, 128, 12416)),
    "code32": ((L3, dict(code=32)), DMA(2, 3, 448, 128, 16640)),
    "code128": ((L3, dict(code=128)), DMA(2, 4, 448, 128, 20736, PIPE=1, TRACE=1)),
    "code128-untraced-plan": (((0, 4, 128, 128, 112), dict(code=128)), RG(4, 3, 1, 448, 256, 24832, route="dma")),
    "code1142": ((L3, dict(code=1142)), KW2_64),
    "code1142-L1": (((1, 1, 32, 32, 576), dict(code=1142)), SP(4, 1, 1, (144, 1, 1), 256, 32768)),
    "code1142-L6": (((0, 6, 128, 128, 48), dict(code=1142)), SP(4, 2, 1, (16, 2, 1), 256, 40960)),
    "code1142-bf16": ((L3, dict(code=1142, bf16=1)), RG(2, 4, 2, 224, 128, 24704)),
    "code1182": (((0, 1, 32, 32, 576), dict(code=1182)), SP(8, 1, 1, (72, 1, 1), 512, 57344)),
    "code1182-64to64": (((0, 2, 64, 64, 352), dict(code=1182)), SP(8, 1, 1, (48, 2, 1), 512, 57344)),
    "code1183": (((0, 1, 32, 32, 576), dict(code=1183)), RES(8, 72, 512, 159744)),
    "code1183-8slot": (((1, 2, 32, 32, 352), dict(code=1183)), RES(8, 48, 512, 81920)),
    "code1542": (((0, 2, 64, 64, 352), dict(code=1542)), SP(4, 2, 1, (88, 1, 1), 256, 40960)),
    "code1942": (((0, 2, 64, 128, 10000), dict(code=1942)), SP(4, 2, 1, (2504, 2, 1), 256, 40960)),
    "code1142-big": (((0, 2, 64, 128, 10000), dict(code=1142)), SP(4, 4, 1, (2504, 1, 1), 256, 57344)),
    "code9142": (((0, 5, 128, 128, 64), dict(code=9142)), SP(4, 1, 2, (16, 4, 1), 512, 65536)),
    "code9142-L6": (((0, 6, 128, 128, 48), dict(code=9142)), SP(4, 1, 1, (16, 4, 1), 256, 32768)),
    "code10142-traced": (((0, 1, 32, 32, 576), dict(code=10142)), SP(4, 1, 1, (144, 1, 1), 256, 32768, TRACE=1)),
    "code10142-traced-128": (((0, 6, 128, 128, 48), dict(code=10142)), SP(4, 2, 1, (16, 2, 1), 256, 40960, TRACE=1)),
}


@pytest.mark.parametrize("name", list(CASES))
def test_thresholds_offset_parts_and_debug_codes(choice, name):
    (layer, settings), want = CASES[name]
    assert choice(*layer, **settings) == want


@pytest.mark.parametrize("code", [3, 64, 999, -1])
def test_unknown_code_below_1000_is_the_product_choice(choice, code):
    for row in LAYERS:
        kind, level, cin, cout = row[0]
        assert choice(kind, level, cin, cout, GROUPS[level], gated=(kind, level) == (1, 2), code=code) == row[1]


STATE, INVALID = 4, 1
REFUSED = {
    "cfg-without-instantiation": ((L3, dict(code=2009)), INVALID, r"sconv\(split\): no instantiation for 64->64 cfg 1009"),
    "cfg-162": ((L3, dict(code=1162)), INVALID, r"sconv\(split\): no instantiation for 64->64 cfg 162"),
    "traced-resident": (((0, 1, 32, 32, 576), dict(code=10183)), INVALID, r"sconv\(split\): no instantiation for 32->32 cfg 9183"),
    "traced-32to64": (((0, 2, 32, 64, 352), dict(code=10142)), INVALID, r"sconv\(split\): no instantiation for 32->64 cfg 9142"),
    "resident-off-32to32": (((0, 2, 32, 64, 352), dict(code=1183)), INVALID,
                            r"the weight-resident form exists for the unsplit 32->32 plan only \(32->64, K 27\)"),
    "resident-offset-parts": (((1, 1, 32, 32, 576), dict(kparts=2)), INVALID,
                              r"the weight-resident form exists for the unsplit 32->32 plan only \(32->32, K 8\)"),
    "gated-cfg": (((1, 2, 32, 32, 352), dict(gated=1, code=1182)), INVALID, r"the gated input exists for the 32->32 plan only"),
    "gated-64": (((1, 3, 64, 64, 224), dict(gated=1)), INVALID, r"the gated input exists for the 32->32 plan only"),
    "gated-split-input": (((1, 2, 32, 32, 352), dict(gated=1, split_io=1)), INVALID, r"the gated input exists for the 32->32 plan only"),
    "gated-resident-k3": (((0, 1, 32, 32, 576), dict(gated=1, code=1183)), INVALID, r"the gated resident form exists for the 8-slot maps"),
    "offset-parts-nw8": ((L3, dict(code=1182)), INVALID, r"no offset-split instantiation for 64->64 \(parts 1, kw 2\)"),
    "offset-parts-32": (((0, 1, 32, 32, 576), dict(kparts=2)), INVALID, r"no offset-split instantiation for 32->32 \(parts 2, kw 0\)"),
    "residual-bf16": (((0, 6, 128, 128, 48), dict(bf16=1, residual=1)), INVALID,
                      r"the epilogue residual exists in the per-tile kernel of fp32 maps \(levels >= 5\) and in the split kernel"),
    "residual-L4-exact": (((0, 4, 128, 128, 112), dict(split_max_level=-1, residual=1)), INVALID, r"the epilogue residual exists in"),
    "residual-two-groups": (((0, 6, 128, 128, 48), dict(code=8, residual=1)), INVALID, r"the epilogue residual exists in"),
    "split-io-tail-split": (((0, 6, 128, 128, 48), dict(split_io=2)), STATE,
                            r"split-form maps and gated inputs are read and written by the split kernel only"),
    "split-io-bf16": ((L3, dict(bf16=1, split_io=1)), STATE, r"split-form maps and gated inputs are read and written by the split kernel only"),
    "gated-exact": (((1, 2, 32, 32, 352), dict(gated=1, split_max_level=-1)), STATE, r"read and written by the split kernel only"),
}


@pytest.mark.parametrize("name", list(REFUSED))
def test_refusals_keep_their_error(choice, name):
    from egonn_amd._lib import EgonnError
    (layer, settings), code, text = REFUSED[name]
    with pytest.raises(EgonnError, match=text) as e:
        choice(*layer, **settings)
    assert e.value.code == code


def test_allowed_extras(choice):
    """what the refusals leave: the residual on the tail levels (product rule, register ring) and on the split route, split-form
    I/O on the split route — none changes the launch"""
    assert choice(0, 6, 128, 128, 48, residual=1) == TAIL
    assert choice(0, 6, 128, 128, 48, residual=1, split_max_level=-1) == RG6
    assert choice(0, 6, 128, 128, 48, residual=1, code=2) == RG6
    assert choice(0, 5, 128, 128, 64, residual=1, split_io=3) == L5_KW2


def test_bad_arguments(choice):
    from egonn_amd._lib import EgonnError
    for layer in ((3, 1, 32, 32, 576), (0, 8, 32, 32, 576), (0, -1, 32, 32, 576), (0, 1, 0, 32, 576), (0, 1, 32, 32, -1)):
        with pytest.raises(EgonnError, match="debug_sconv_choice: bad arguments"):
            choice(*layer)


def test_environment_switches_go_through_the_same_decoder():
    """EGONN_SPLIT_CFG is decoded like the cfg of code 1000 + cfg (and gives way to it); EGONN_SPLIT_MAX_LEVEL_K8 is the limit of
    the 8-slot maps alone.  The switches are read once per process: a child process, host only."""
    prog = ("from egonn_amd import _lib; c = _lib.debug_sconv_choice\n"
            "f = lambda d: (d['route'], d['NW'], d['NSW'], d['KW'], d['resident'], d['gx'], d['gy'], d['block'], d['lds'])\n"
            "print(f(c(0, 1, 32, 32, 576)), f(c(1, 1, 32, 32, 576)), f(c(0, 1, 32, 32, 576, code=1142)),\n"
            "      f(c(1, 2, 32, 32, 352)), f(c(0, 2, 32, 64, 352)))")
    env = dict(os.environ, EGONN_SPLIT_CFG="182", EGONN_SPLIT_MAX_LEVEL_K8="1")
    out = subprocess.run([sys.executable, "-c", prog], cwd=REPO, env=env, capture_output=True, text=True, check=True).stdout
    assert out.strip() == " ".join(str(t) for t in (
        ("split", 8, 1, 1, 0, 72, 1, 512, 57344),       # cfg 182 from the environment: workgroups of 8 waves
        ("split", 8, 1, 1, 0, 72, 1, 512, 57344),       # ... no resident rule under a cfg other than 142; an 8-slot map at its limit 1
        ("split", 4, 1, 1, 0, 144, 1, 256, 32768),      # the setting's own cfg wins
        ("dma", 1, 0, 0, 0, 352, 1, 64, 10368),         # 8-slot map above its limit: an exact kernel
        ("split", 8, 1, 1, 0, 48, 2, 512, 57344)))      # the k=3 map of the same level keeps the context's limit
