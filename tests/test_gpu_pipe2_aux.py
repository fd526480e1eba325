"""GPU-box test of the target map built inside the pair launch (``DCPipeline(aux_map=True)``, onssen_blstm_pipe2_map_forward_f32: the
launch's trailing workgroups) against the parent's launch sequence (``aux_map=False``: onssen_dc_index_f32 in front of the launch).
Same model, same batches, both pipelines side by side: equal masks, equal waveforms, byte-equal clustering workspaces after every push."""
import numpy as np
import pytest
import torch

from onssen_amd.synthetic import make_state_dict, synth_mixture

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from onssen_amd.hip import get_lib
    get_lib()
    return torch.device("cuda:0")


def _dc(dev, H, seed, F=129, D=20):
    from onssen_amd import nn as onn
    sd = make_state_dict("deep_clustering", F, H, 2, D, 2, seed=seed)
    m = onn.deep_clustering(F, H, 2, D)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    return m.to(dev).eval()


# (64, 32, 64 * 130): T = 131, 16 899 bins per utterance -- the smallest size at which one of the 64 chunks exceeds 256 bins, so that
# kmeans2_index_kernel's scan takes a second round; every aux workgroup owns two utterances there
@pytest.mark.parametrize("H,B,n,graph", [(32, 5, 64 * 24, False), (64, 20, 64 * 37, True), (64, 32, 64 * 130, True)])
def test_aux_map_equals_the_three_launches_in_front(dev, H, B, n, graph):
    from onssen_amd.nn import _core
    from onssen_amd.separation import DCPipeline
    m = _dc(dev, H, seed=H + B)
    xs = [torch.from_numpy(np.stack([synth_mixture(500 + 97 * k + b, n) for b in range(B)])).to(dev) for k in range(4)]
    a0 = _core._XcdPolicy.aborts
    new, old = DCPipeline(m, B, n, graph=graph, aux_map=True), DCPipeline(m, B, n, graph=graph, aux_map=False)
    assert new.aux_map and not old.aux_map
    torch.cuda.synchronize()
    for q in (0, 1):          # the same starting bytes, whatever the allocator handed out behind the zeroed headers
        old.cws[q].copy_(new.cws[q])
    old.masks.copy_(new.masks)

    def status_words(p):
        return [int(p.ws.view(torch.int32)[280])] + [int(p.cws[q][p.cstat:p.cstat + 4].view(torch.int32)[0]) for q in (0, 1)]

    def compare(k, out_new, out_old):
        torch.cuda.synchronize()
        for q in (0, 1):
            assert torch.equal(new.cws[q], old.cws[q]), (k, q)
        assert status_words(new) == [0, 0, 0] and status_words(old) == [0, 0, 0], k
        if out_new is None:
            assert out_old is None
            return
        assert torch.equal(new.masks, old.masks), k
        assert torch.isfinite(out_new).all() and torch.equal(out_new, out_old), k

    for k, x in enumerate(xs):
        compare(k, new.push(x), old.push(x))
    compare(4, new.flush(), old.flush())
    _core._XcdStatus.flush()
    assert _core._XcdPolicy.aborts == a0
    assert new.masks.sum() > 0
