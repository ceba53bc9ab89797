"""The <8,8> evaluator's 64-column layers (the stem and every block's last 1x1) may carry a wave's tiles in two GROUPS (ccsp_net.hip:
gemm_tiles_grouped, CCSP_NET_TILE_GROUPS / _STEM) -- the order BETWEEN tiles changes, no chain does: the forced <8,8> shape gives the bits
of the forced <2,8> shape (which has one or two tiles per wave in these layers and none of that code), and the request form gives the
bits of the planes path.  Holds before and after the grouping (it passes on the ungrouped kernel as well).

Batch sizes: 1 (a lone row), 8 (a full workgroup: every tile of both groups of both row halves live, the tile fed from Smem::part among
them), 9 (a full workgroup and one with ONE real position) and 17 (two full and one with one): in a part-filled workgroup every tile
holds only some real rows.  Nets: good_model.h5 and a seeded random-weight net (scaled as in tests/test_gpu_net_tail_tile.py)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = (1, 8, 9, 17)
NETS = ('good_model', 'random')


def _model(name, golden_dir):
    import torch
    from chinesecheckersagent_amd.model import ResidualCNN
    m = ResidualCNN(device='cuda', backend='hip')
    if name != 'random':
        m.load_weights(golden_dir + '/%s.h5' % name)
        return m
    rng = np.random.RandomState(20)                    # He-scaled normal weights, biases of the activations' size
    with torch.no_grad():
        for mod in m.model.modules():
            w = getattr(mod, 'weight', None)
            if w is None:
                continue
            fan_in = int(np.prod(w.shape[1:]))
            w.copy_(torch.from_numpy((rng.standard_normal(tuple(w.shape)) * np.sqrt(2.0 / fan_in)).astype(np.float32)))
            mod.bias.copy_(torch.from_numpy((rng.standard_normal(tuple(mod.bias.shape)) * 0.1).astype(np.float32)))
    m._packed = None
    return m


def _forward(m, x):
    lg, v = m.predict_batch(x)
    p, v2 = m.evaluate_batch(x)
    return lg, v, p, v2


@pytest.mark.parametrize('name', NETS)
def test_gpu_shape_8_equals_shape_2(name, golden_dir):
    """logits, v and p of the forced <8,8> shape == those of the forced <2,8> shape, 1 / 8 / 9 / 17 positions"""
    import torch
    from chinesecheckersagent_amd import _lib
    L = _lib.lib()
    m = _model(name, golden_dir)
    base = torch.from_numpy(np.load(golden_dir + '/net.npz')['planes'][:max(SIZES)].astype(np.float32)).cuda()
    try:
        assert L.ccsp_debug_net_shape(2) == 2
        want = _forward(m, base)                       # the reference: computed once
        assert all(bool(torch.isfinite(t).all()) for t in want) and torch.equal(want[1], want[3])
        assert float(want[0].abs().max()) > 0 and len(torch.unique(want[0][:, 0])) > max(SIZES) // 2     # (not one evaluation 17 times)
        assert L.ccsp_debug_net_shape(8) == 8
        for n in SIZES:
            got = _forward(m, base[:n].contiguous())
            for g, w, what in zip(got, want, ('logits', 'v', 'p', 'v of the softmax call')):
                assert torch.equal(g, w[:n]), (name, what, n)
    finally:
        L.ccsp_debug_net_shape(0)


@pytest.mark.parametrize('name', NETS)
def test_gpu_request_form_equals_planes_path(name, golden_dir):
    """ccsp_net_forward_requests in the forced <8,8> shape == encode -> ccsp_net_forward in the forced <2,8> shape -> gather, on the first
    1 / 8 / 9 / 17 of 17 request records (every one asks; move rows of 1 .. CCSP_MAX_MOVES entries); what nobody asked for stays"""
    import torch
    from chinesecheckersagent_amd import _lib
    from chinesecheckersagent_amd.model import evaluate_requests_with
    L = _lib.lib()
    z = np.load(golden_dir + '/rules.npz')
    N = max(SIZES)
    rng = np.random.RandomState(11)
    pick = rng.choice(len(z['pos12']), N, replace=False)
    req = np.zeros(N, dtype=_lib.REQUEST_DTYPE)
    req['state'] = _lib.pack_states(z['pos12'][pick], z['last'][pick])
    req['player'] = z['player'][pick]
    ks = np.array([1, 63, 64, 65, _lib.MAX_MOVES])[np.arange(N) % 5]
    req['k'] = ks
    req['kind'] = 1 + 2 * (np.arange(N) % 2)
    moves = rng.randint(0, _lib.NUM_ACTIONS, size=(N, _lib.REQUEST_MOVES)).astype(np.uint16)
    d_req = torch.from_numpy(req.view(np.uint8).reshape(N, 64)).cuda()
    d_mv = torch.from_numpy(moves.view(np.int16)).cuda()
    m = _model(name, golden_dir)
    live = torch.arange(_lib.REQUEST_MOVES, device='cuda')[None, :] < torch.from_numpy(ks.astype(np.int64)).cuda()[:, None]
    try:
        assert L.ccsp_debug_net_shape(2) == 2
        want_pk = torch.full((N, _lib.REQUEST_MOVES), -7.0, dtype=torch.float64, device='cuda')
        want_pk, want_v = evaluate_requests_with(m.evaluate_batch, d_req, d_mv, want_pk)       # the reference: computed once
        torch.cuda.synchronize()
        assert (want_pk[~live] == -7.0).all() and bool((want_pk[live] >= 0).all()) and float(want_pk[live].sum()) > 0
        assert len(torch.unique(want_pk[:, 0])) > N // 2      # (not one evaluation 17 times; the random net's v is one value: its value head is dead)
        assert L.ccsp_debug_net_shape(8) == 8
        for n in SIZES:
            pk = torch.full((n, _lib.REQUEST_MOVES), -7.0, dtype=torch.float64, device='cuda')
            v = torch.full((n,), -7.0, dtype=torch.float32, device='cuda')
            m.evaluate_requests(d_req[:n].contiguous(), d_mv[:n].contiguous(), pk, v)
            torch.cuda.synchronize()
            assert torch.equal(pk[live[:n]], want_pk[:n][live[:n]]), (name, n)
            assert (pk[~live[:n]] == -7.0).all() and torch.equal(v, want_v[:n]), (name, n)
    finally:
        L.ccsp_debug_net_shape(0)
