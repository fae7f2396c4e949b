"""GPU test of the work-arena claim (csrc/model.hip: claim_work): whoever resets a context's work arena retires what pointed
into it.  After an egonn_forward the level maps are readable; every operator entry point that claims the arena must leave
egonn_forward_level_features answering EGONN_ERR_STATE, and a forward after all of them is bitwise the first one."""
import pytest
import torch

from tests import helpers as H

pytestmark = pytest.mark.gpu


def test_every_claiming_operator_retires_the_forward_maps():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import __graft_entry__ as g
    g.build()
    import egonn_amd
    from egonn_amd import _lib
    from egonn_amd.synth import lidar_scan

    m = egonn_amd.model_factory(egonn_amd.ModelParams(model="egonn", coordinates="cartesian", quantization_step=0.1))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in H.seeded_weights(11).items()})
    m = m.to("cuda").eval()
    m.coord_bits = 12
    ctx = m.context()
    scans = [torch.from_numpy(lidar_scan(70 + i, 300)) for i in range(2)]
    pts, off = torch.cat(scans).cuda().contiguous(), [0, len(scans[0]), len(scans[0]) + len(scans[1])]
    ctx.voxelize(pts, off, m.quantizer.mode, m.quantizer.step)
    ctx.keep_level_features(True)

    def forward():
        with torch.no_grad():
            y = m._forward_on_plan(ctx, None)
        out = [y["global"]] + list(m._last_local)
        assert ctx.forward_level_features(1, 32).shape == (n[1], 32)        # the maps of this forward are there
        return [t.clone() for t in out]

    n = [ctx.level_count(l) for l in range(8)]
    assert all(v >= 1 for v in n)
    gen = torch.Generator(device="cuda").manual_seed(3)
    rand = lambda *s: torch.randn(*s, device="cuda", generator=gen)      # noqa: E731
    x3, x1 = rand(n[3], 64), rand(n[1], 32)
    bn = lambda c: torch.nn.BatchNorm1d(c).cuda()                          # noqa: E731
    lens = ctx.level_batch_offsets(3)
    nmax = max(lens[b + 1] - lens[b] for b in range(2))
    wc, w2, hid = rand(64, 64) * 0.1, rand(1, 64, 64) * 0.1, rand(64 * 64, 128) * 0.02
    operators = {
        "gem": lambda: ctx.gem(3, x3.abs(), torch.tensor([3.0])),
        "global_max_pool": lambda: ctx.global_max_pool(3, x3),
        "global_avg_pool": lambda: ctx.global_avg_pool(3, x3),
        "block_tail": lambda: ctx.block_tail(3, x3, x3, rand(1, 1, 3)),
        "netvlad": lambda: ctx.netvlad(3, x3, wc, w2, bn(64), hid, bn(128)),
        "conv": lambda: ctx.conv(1, 1, 3, x1, rand(27, 32, 32) * 0.05),
        "topdown_step": lambda: ctx.topdown_step(3, rand(n[4], 64), rand(8, 64, 64) * 0.05, x3, rand(64, 64) * 0.1),
        "netvlad_train_forward": lambda: ctx.netvlad_train_forward(3, x3, nmax, wc, w2, bn(64), hid),
    }
    try:
        saved = forward()
        for name, op in operators.items():
            if name != "gem":
                forward()
            op()
            with pytest.raises(_lib.EgonnError) as ei:
                ctx.forward_level_features(3, 64)
            assert ei.value.code == 4, name
        ctx.plan_status()
        again = forward()
    finally:
        ctx.keep_level_features(False)
    assert len(saved) == 4 and all(torch.equal(a, b) for a, b in zip(saved, again))
