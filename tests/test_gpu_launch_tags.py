"""The profiler tag of every sparse convolution of egonn_forward names the kernel that runs, in the order it runs: bench.py's
roofline leg keys on it.  One eager forward of the smoke batch (2 scans of 6000 points, Cartesian step 0.1 m, seeded weights) per
setting — the fp32 product rule, fp32 on the exact kernels (set_exact_fp32) and bf16 maps — and the ordered names of
profile_fetch() must equal tests/golden/forward_launch_tags.json: the recorded launch order of that forward, each tag of the
form <kernel><cin,cout>/L<level>/<layer> with <kernel> the kernel sconv_map dispatches for the layer."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "forward_launch_tags.json")
SETTINGS = ("fp32", "fp32_exact", "bf16")


def launch_tags():
    """{setting: ordered launch names of one eager egonn_forward on the smoke batch}"""
    import __graft_entry__ as entry
    entry.build()
    import egonn_amd as E
    from egonn_amd.synth import lidar_scan, seeded_state_dict
    model = E.model_factory(E.ModelParams(model="egonn", coordinates="cartesian", quantization_step=0.1))
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_state_dict(7, shapes).items()})
    model = model.to("cuda:0").eval()
    scans = [lidar_scan(2 + i, n_points=6000) for i in range(2)]
    off = [0, len(scans[0]), len(scans[0]) + len(scans[1])]
    pts = torch.from_numpy(np.concatenate(scans)).cuda()
    ex = E.DescriptorExtractor(model, n_k=128)
    ctx = model.context(0)
    tags = {}
    for setting in SETTINGS:
        model.precision = "bf16" if setting == "bf16" else "fp32"
        ctx.set_exact_fp32(setting == "fp32_exact")
        ctx.profile_enable(1)
        ex.extract_packed(pts, off)
        tags[setting] = [r[0] for r in ctx.profile_fetch()]
        ctx.profile_enable(0)
    ctx.set_exact_fp32(False)
    return tags


@pytest.fixture(scope="module")
def tags():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return launch_tags()


@pytest.mark.parametrize("setting", SETTINGS)
def test_forward_launch_tags(tags, setting):
    with open(GOLDEN) as f:
        want = json.load(f)[setting]
    assert len(want) > 0
    assert tags[setting] == want
