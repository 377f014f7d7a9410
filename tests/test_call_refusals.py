"""The two holes the typed call boundary closes, on the GPU at the smallest legal shapes: a refused call raises before the
library is entered, so nothing is launched and nothing is written."""
import numpy as np
import pytest
import torch

from oracle import gatsspg_oracle as orc
from onepose_amd import GATsSuperGlue, SuperGlue, synthetic

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SENTINEL = -77


def load(module, sd):
    module.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}, strict=True)
    return module.eval().to(DEV)


def test_superglue_refuses_int32_match_buffers_and_leaves_them_alone():
    """The kernel stores int64 into matches0 / matches1: int32 buffers of the right shape used to be overrun silently."""
    b, n0, n1, hw = 1, 3, 4, (48, 64)
    engine = load(SuperGlue({"GNN_layers": ["self"]}), synthetic.make_superglue_state_dict(7, 1)).engine
    g = torch.Generator().manual_seed(3)
    side = lambda n: (torch.rand(b, n, 2, generator=g) * 40 + 2, torch.rand(b, n, generator=g),  # noqa: E731
                      torch.nn.functional.normalize(torch.randn(b, 256, n, generator=g), dim=1))
    inputs = [t.to(DEV) for t in side(n0) + side(n1)]
    ref = engine.forward(*inputs, hw, hw)

    bad = (torch.full((b, n0), SENTINEL, device=DEV, dtype=torch.int32), torch.full((b, n1), SENTINEL, device=DEV, dtype=torch.int32),
           torch.full((b, n0), float(SENTINEL), device=DEV), torch.full((b, n1), float(SENTINEL), device=DEV))
    with pytest.raises(TypeError, match="sg_forward argument 18:"):
        engine.forward(*inputs, hw, hw, out=bad)
    torch.cuda.synchronize()
    assert all(bool((t == SENTINEL).all()) for t in bad)

    good = engine.outputs(b, n0, n1, DEV)
    for t in good:
        t.fill_(SENTINEL)
    got = engine.forward(*inputs, hw, hw, out=good)
    assert all(g_ is o for g_, o in zip(got, good)) and all(torch.equal(a, r) for a, r in zip(got, ref))


def test_gatsspg_stage_refuses_a_strided_leaf_tensor():
    b, n1, n2, num_leaf = 1, 2, 2, 1
    engine = load(GATsSuperGlue(dict(orc.DEFAULT_HPARAMS)), synthetic.make_state_dict(0)).engine
    dq, d3 = torch.randn(b, 256, n1, device=DEV), torch.randn(b, 256, n2, device=DEV)
    dims = engine.load_state(dq, d3, num_leaf)
    d2db = torch.randn(b, n2 * num_leaf, 256, device=DEV).transpose(1, 2)       # [b,256,n2*num_leaf], channel stride 1
    assert d2db.shape == (b, 256, n2 * num_leaf) and not d2db.is_contiguous()
    with pytest.raises(TypeError, match="gatsspg_gats_layer argument 2:"):
        engine.gats_layer(dims, 0, d2db)
    engine.gats_layer(dims, 0, d2db.contiguous())                                # the same values, laid out as the header says
    torch.cuda.synchronize()
