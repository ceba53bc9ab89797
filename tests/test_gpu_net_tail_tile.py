"""The fused evaluator's <8,8> shape against the shapes that share none of its 3x3 code, and its compact (request) answer against the
planes path -- bit for bit.  These pin the ARITHMETIC: <8,8> computes the 25th cell's tile of the 3x3 layers on another instruction
(v_mfma_f32_4x4x1, ccsp_net.hip: tail_tile_4x4) than <2,8> and <1,8> (v_mfma_f32_16x16x4), and the request form divides only the
softmax entries that are picked; every result must stay what the other shapes / the planes path give."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FILES = ('good_model', 'good_model2', 'version0016-weights')
NETS = FILES + ('random', 'random_x64')


@pytest.fixture(scope='module')
def planes24(golden_dir):
    return np.load(golden_dir + '/net.npz')['planes'][:24].astype(np.float32)


def _model(name, golden_dir):
    """one of the reference's weight files, or a seeded random net (He-scaled normal weights, biases of the activations' size);
    'random_x64': the stem 64 times larger, so that every activation of the trunk is"""
    import torch
    from chinesecheckersagent_amd.model import ResidualCNN
    m = ResidualCNN(device='cuda', backend='hip')
    if name in FILES:
        m.load_weights(golden_dir + '/%s.h5' % name)
        return m
    rng = np.random.RandomState(20 if name == 'random' else 21)
    with torch.no_grad():
        for mod in m.model.modules():
            w = getattr(mod, 'weight', None)
            if w is None:
                continue
            fan_in = int(np.prod(w.shape[1:]))
            scale = 64.0 if (name == 'random_x64' and mod is m.model.stem) else 1.0
            w.copy_(torch.from_numpy((rng.standard_normal(tuple(w.shape)) * np.sqrt(2.0 / fan_in) * scale).astype(np.float32)))
            mod.bias.copy_(torch.from_numpy((rng.standard_normal(tuple(mod.bias.shape)) * 0.1 * scale).astype(np.float32)))
    m._packed = None
    return m


def _forward(m, x):
    lg, v = m.predict_batch(x)
    p, v2 = m.evaluate_batch(x)
    return lg, v, p, v2


@pytest.mark.parametrize('name', NETS)
def test_gpu_shape_8_equals_shapes_2_and_1(name, planes24, golden_dir):
    """24 positions, each once in every one of the 8 slots of a workgroup (the eight rotations of every group of eight), batches of 8,
    11 (a ragged last workgroup) and 24: logits, v and p of the forced <8,8> shape are the bits of the forced <2,8> and <1,8> shapes"""
    import torch
    from chinesecheckersagent_amd import _lib
    L = _lib.lib()
    m = _model(name, golden_dir)
    base = torch.from_numpy(planes24).cuda()
    try:
        assert L.ccsp_debug_net_shape(2) == 2
        want = _forward(m, base)                       # the reference: computed once, in the positions' own order
        assert L.ccsp_debug_net_shape(1) == 1
        for a, b in zip(_forward(m, base), want):
            assert torch.equal(a, b)
        assert all(bool(torch.isfinite(t).all()) for t in want) and torch.equal(want[1], want[3])
        assert float(want[0].abs().max()) > 0 and len(torch.unique(want[0][:, 0])) > 12       # (not one evaluation 24 times)
        assert L.ccsp_debug_net_shape(8) == 8
        i = torch.arange(24)
        for rot in range(8):
            perm = (8 * (i // 8) + (i % 8 - rot) % 8).cuda()        # batch row -> position: position p stands in slot (p + rot) % 8
            for n in (8, 11, 24):
                got = _forward(m, base[perm[:n]].contiguous())
                for g, w, what in zip(got, want, ('logits', 'v', 'p', 'v of the softmax call')):
                    assert torch.equal(g, w[perm[:n]]), (name, what, rot, n)
    finally:
        L.ccsp_debug_net_shape(0)


def test_gpu_compact_answer_equals_planes_path(golden_dir):
    """ccsp_net_forward_requests == ccsp_encode_requests -> ccsp_net_forward -> ccsp_gather_priors on 19 request records (two full
    workgroups of <8,8> and a ragged third, rows of kind 0 in between), move rows of 1, 63, 64, 65 and CCSP_MAX_MOVES entries (both
    halves of the pick), one entry that is no action index (answers 0.0); rows and entries nobody asked for stay untouched"""
    import torch
    from chinesecheckersagent_amd import _lib
    from chinesecheckersagent_amd.model import ResidualCNN, evaluate_requests_with
    L = _lib.lib()
    z = np.load(golden_dir + '/rules.npz')
    n = 19
    rng = np.random.RandomState(7)
    pick = rng.choice(len(z['pos12']), n, replace=False)
    req = np.zeros(n, dtype=_lib.REQUEST_DTYPE)
    req['state'] = _lib.pack_states(z['pos12'][pick], z['last'][pick])
    req['player'] = z['player'][pick]
    ks = np.array([1, 63, 64, 65, _lib.MAX_MOVES])[np.arange(n) % 5]
    req['k'] = ks
    req['kind'] = np.where(np.isin(np.arange(n), (2, 9, 17)), 0, 1 + 2 * (np.arange(n) % 2))      # kinds 1 and 3 ask, 0 does not
    moves = rng.randint(0, _lib.NUM_ACTIONS, size=(n, _lib.REQUEST_MOVES)).astype(np.uint16)
    moves[:, ::5] |= 0x8000                                        # (the "wins" mark is not part of the index)
    moves[4, 70] = 300                                             # no action index (row 4: CCSP_MAX_MOVES entries, second half of the pick)
    moves[1, 10] = 294 | 0x8000
    d_req = torch.from_numpy(req.view(np.uint8).reshape(n, 64)).cuda()
    d_mv = torch.from_numpy(moves.view(np.int16)).cuda()
    m = ResidualCNN(device='cuda', backend='hip')
    m.load_weights(golden_dir + '/good_model.h5')
    want_pk = torch.full((n, _lib.REQUEST_MOVES), -7.0, dtype=torch.float64, device='cuda')
    want_pk, want_v = evaluate_requests_with(m.evaluate_batch, d_req, d_mv, want_pk)
    asks = torch.from_numpy(req['kind'] != 0).cuda()
    live = (torch.arange(_lib.REQUEST_MOVES, device='cuda')[None, :] < torch.from_numpy(ks.astype(np.int64)).cuda()[:, None]) & asks[:, None]
    assert (want_pk[~live] == -7.0).all() and float(want_pk[4, 70]) == 0.0 and float(want_pk[1, 10]) == 0.0
    assert int(live.sum()) == int(ks[req['kind'] != 0].sum()) and int((want_pk[live] > 0).sum()) == int(live.sum()) - 2
    for shape in (8, 4, 2, 1, 0):
        L.ccsp_debug_net_shape(shape)
        try:
            pk = torch.full((n, _lib.REQUEST_MOVES), -7.0, dtype=torch.float64, device='cuda')
            v = torch.full((n,), -7.0, dtype=torch.float32, device='cuda')
            m.evaluate_requests(d_req, d_mv, pk, v)
            torch.cuda.synchronize()
        finally:
            L.ccsp_debug_net_shape(0)
        assert torch.equal(pk[live], want_pk[live]), shape
        assert (pk[~live] == -7.0).all() and torch.equal(v[asks], want_v[asks]) and (v[~asks] == -7.0).all(), shape
