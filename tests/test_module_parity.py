"""Parity of the drop-in modules against the reference's golden vectors, on two kernel sets.

``dev = cpu-emulated`` (always runs) -- CPU check of the HOST LOGIC: the launch sequences in
``stc_hip.ops`` and the drop-in modules of ``STC_GNN.py`` reproduce the reference's golden
vectors when the kernels are stood in for by ``oracle/kernel_emul.py`` (test infrastructure,
injected here; the product has no CPU path).  This proves, before any GPU time is spent, that
the decomposition the HIP path uses -- feature-side Chebyshev recurrence over CSR operands,
project-then-mix node kernel, hand-derived backward incl. dGs/dGc, fused gate math, module
wiring and state_dict keys -- is the reference's math.

``dev = cuda`` (marked gpu) -- the same cases through libstc_hip.so on the MI355X: the drop-in
modules against the reference's goldens, forward and every gradient, tolerance 1e-5 relative
(north_star: "match the reference PyTorch-CPU forward ... to <=1e-5 relative fp32"; relative =
max|a-b| / max|b|).  Measured errors are appended to gpurun_out/parity_errors.txt.
"""
import os

import pytest
import torch

import STC_GNN as M
from oracle import stc_oracle as O
from oracle.kernel_emul import EmulatedKernels
from stc_hip import CsrGraph, ops
from tests.conftest import REPO, load_golden, rel_err, sub_dict
from tests.golden.make_golden import SF_SHAPE, bench_path_inputs, synth_inputs
from tests.launch_trace import FANOUT_OUTPUTS, FANOUT_SCHEDULE

FWD = 2e-6       # CPU-emulated bound, forward
GRAD = 5e-6      # CPU-emulated bound, gradients
GPU = 1e-5       # bound on the GPU (north_star)
DEV = 'cpu'


@pytest.fixture(autouse=True, params=['cpu-emulated', pytest.param('cuda', marks=pytest.mark.gpu)])
def dev(request, monkeypatch):
    """Select the kernel set: the emulated twin on CPU tensors, or the HIP library on the GPU."""
    global DEV
    if request.param == 'cuda':
        monkeypatch.setattr(ops, '_kernels', None)          # -> HipKernels() on first use; raises if not built
        DEV = 'cuda'
    else:
        monkeypatch.setattr(ops, '_kernels', EmulatedKernels())
        DEV = 'cpu'
    yield DEV
    DEV = 'cpu'


def _close(got, want, cpu_tol, what, gpu_tol=GPU):
    err = rel_err(got, want)
    if DEV == 'cuda':      # keep the measured errors: they feed DESIGN.md's parity table
        out = os.path.join(REPO, 'gpurun_out')
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, 'parity_errors.txt'), 'a') as f:
            f.write(f'{os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0]}\t{what}\t{err:.3e}\n')
    bound = cpu_tol if DEV == 'cpu' else max(cpu_tol, gpu_tol)
    assert err < bound, f'{what}: relative error {err:.3e} >= {bound:.1e}'


def _golden(name):
    return {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in load_golden(name).items()}


def _leaf(t):
    return t.clone().to(DEV).requires_grad_()


@pytest.mark.parametrize('K', [1, 2, 3])
def test_bdg_dif_module_matches_reference_golden(K):
    g = _golden(f'g1_bdg_k{K}')
    B, N, C, L = g['X'].shape
    layer = M.BDG_Dif(K, K, L, g['W'].shape[1]).to(DEV)
    layer.load_state_dict({'W': g['W'], 'b': g['b']})
    X, Gs, Gc = _leaf(g['X']), _leaf(g['Gs']), _leaf(g['Gc'])
    Y = layer(X, Gs, Gc)
    _close(Y, g['Y'], FWD, 'Y')
    (Y * g['R']).sum().backward()
    _close(X.grad, g['dX'], FWD, 'dX')
    _close(layer.W.grad, g['dW'], FWD, 'dW')
    _close(layer.b.grad, g['db'], FWD, 'db')
    if K > 1:
        _close(Gs.grad, g['dGs'], FWD, 'dGs')
        _close(Gc.grad, g['dGc'], FWD, 'dGc')
    else:   # K=1: only T_0 = I is used; the drop-in reports zeros where the reference reports None
        assert Gs.grad is None or float(Gs.grad.abs().max()) == 0.0
        assert Gc.grad is None or float(Gc.grad.abs().max()) == 0.0


def test_bdg_dif_no_bias_and_activation():
    g = _golden('g1_bdg_nobias')
    layer = M.BDG_Dif(2, 2, g['X'].shape[-1], g['W'].shape[1], use_bias=False).to(DEV)
    assert [k for k, _ in layer.state_dict().items()] == ['W']
    layer.load_state_dict({'W': g['W']})
    _close(layer(g['X'], g['Gs'], g['Gc']), g['Y'], FWD, 'Y(no bias)')
    act = M.BDG_Dif(2, 2, g['X'].shape[-1], g['W'].shape[1], use_bias=False, activation=torch.nn.ReLU).to(DEV)
    act.load_state_dict({'W': g['W']})
    _close(act(g['X'], g['Gs'], g['Gc']), torch.relu(g['Y']), FWD, 'relu(Y)')


@pytest.mark.parametrize('cin,K', [(1, 2), (1, 3), (4, 2), (4, 3)])
def test_stc_cell_module(cin, K):
    g = _golden(f'g2_cell_in{cin}_k{K}')
    B, N, C, h = g['Ht'].shape
    cell = M.STC_Cell(N, C, K, K, cin, h).to(DEV)
    cell.load_state_dict(sub_dict(g, 'sd/'))
    Xt, Ht, Gs, Gc = (_leaf(g[k]) for k in ('Xt', 'Ht', 'Gs', 'Gc'))
    out = cell(Gs=Gs, Gc=Gc, Xt=Xt, Ht_1=Ht)
    _close(out, g['Hout'], FWD, 'Ht')
    (out * g['R']).sum().backward()
    for name, leaf in (('dXt', Xt), ('dHt', Ht), ('dGs', Gs), ('dGc', Gc)):
        _close(leaf.grad, g[name], GRAD, name)
    grads = dict(cell.named_parameters())
    for k, v in sub_dict(g, 'grad/').items():
        _close(grads[k].grad, v, GRAD, 'd' + k)


def test_stc_cell_composed_path_with_activation_module():
    """A BDG_Dif activation (Identity here) routes the cell through the composed operator sequence."""
    g = _golden('g2_cell_in4_k3')
    B, N, C, h = g['Ht'].shape
    cell = M.STC_Cell(N, C, 3, 3, 4, h, activation=torch.nn.Identity).to(DEV)
    cell.load_state_dict(sub_dict(g, 'sd/'))
    Xt, Ht, Gs, Gc = (_leaf(g[k]) for k in ('Xt', 'Ht', 'Gs', 'Gc'))
    out = cell(Gs=Gs, Gc=Gc, Xt=Xt, Ht_1=Ht)
    _close(out, g['Hout'], FWD, 'Ht (composed)')
    (out * g['R']).sum().backward()
    for name, leaf in (('dXt', Xt), ('dHt', Ht), ('dGs', Gs), ('dGc', Gc)):
        _close(leaf.grad, g[name], GRAD, name + ' (composed)')


def test_encoder_decoder_modules():
    g = _golden('g3_encdec')
    K, h, layers = int(g['K']), int(g['h']), int(g['layers'])
    B, T, N, C, _ = g['X_seq'].shape
    enc = M.STC_Encoder(N, C, K, K, 1, h, layers, return_all_layers=True).to(DEV)
    enc.load_state_dict(sub_dict(g, 'enc_sd/'))
    X_seq, Gs, Gc = _leaf(g['X_seq']), _leaf(g['Gs']), _leaf(g['Gc'])
    seqs, lasts = enc(Gs=Gs, Gc=Gc, X_seq=X_seq, H0_l=None)
    _close(seqs[0], g['seq0'], FWD, 'enc seq0')
    _close(seqs[1], g['seq1'], FWD, 'enc seq1')
    _close(lasts[1], g['last1'], FWD, 'enc last1')
    ((seqs[0] * g['R0']).sum() + (seqs[1] * g['R1']).sum() + (lasts[0] * g['RL']).sum()).backward()
    _close(X_seq.grad, g['dX_seq'], GRAD, 'enc dX_seq')
    _close(Gs.grad, g['enc_dGs'], GRAD, 'enc dGs')
    _close(Gc.grad, g['enc_dGc'], GRAD, 'enc dGc')
    grads = dict(enc.named_parameters())
    for k, v in sub_dict(g, 'enc_grad/').items():
        _close(grads[k].grad, v, GRAD, 'enc d' + k)
    enc.return_all_layers = False
    s2, l2 = enc(g['Gs'], g['Gc'], g['X_seq'])
    assert len(s2) == 1 and len(l2) == 1
    _close(s2[0], g['seq_last_only'], FWD, 'enc last-layer-only')

    dec = M.STC_Decoder(N, C, K, K, h, h, layers, out_horizon=2).to(DEV)
    dec.load_state_dict(sub_dict(g, 'dec_sd/'))
    Gs, Gc, Xd = _leaf(g['Gs']), _leaf(g['Gc']), _leaf(g['Xd'])
    H0 = [_leaf(g['H00']), _leaf(g['H01'])]
    top, states = dec(Gs=Gs, Gc=Gc, Xt=Xd, H0_l=H0)
    _close(top, g['dec_top'], FWD, 'dec top')
    _close(states[0], g['dec_s0'], FWD, 'dec state0')
    ((top * g['Rd']).sum() + (states[0] * g['Rs']).sum()).backward()
    _close(Xd.grad, g['dXd'], GRAD, 'dec dXt')
    _close(H0[0].grad, g['dH00'], GRAD, 'dec dH0[0]')
    _close(H0[1].grad, g['dH01'], GRAD, 'dec dH0[1]')
    _close(Gs.grad, g['dec_dGs'], GRAD, 'dec dGs')
    _close(Gc.grad, g['dec_dGc'], GRAD, 'dec dGc')
    grads = dict(dec.named_parameters())
    for k, v in sub_dict(g, 'dec_grad/').items():
        _close(grads[k].grad, v, GRAD, 'dec d' + k)


def _small_model(g, **kw):
    return M.STCGNN(num_nodes=int(g['N']), num_categories=int(g['C']), Ks=int(g['K']), Kc=int(g['K']), input_dim=1,
                    hidden_dim=int(g['h']), num_layers=int(g['layers']), out_horizon=int(g['horizon']), **kw).to(DEV)


def test_full_model_state_dict_keys_loss_and_grads():
    g = _golden('g4_stcgnn_small')
    model = _small_model(g)
    sd = sub_dict(g, 'sd/')
    assert list(model.state_dict().keys()) == list(sd.keys())        # same keys, same order as the reference
    for k, v in model.state_dict().items():
        assert tuple(v.shape) == tuple(sd[k].shape), k
    model.load_state_dict(sd)
    Gs, Gc = model.mix_graph_pair(g['X'], g['As'], g['Ac'])
    _close(Gs, g['Gs'], FWD, 'MGP_Gen Gs')
    _close(Gc, g['Gc'], FWD, 'MGP_Gen Gc')
    yhat = model(X_seq=g['X'], As=g['As'], Ac=g['Ac'])
    assert yhat.shape == g['yhat'].shape
    _close(yhat, g['yhat'], FWD, 'yhat')
    loss = O.combo_loss(yhat, g['Y'])
    assert abs(float(loss.detach()) - float(g['loss'])) < 2e-6
    loss.backward()
    grads = dict(model.named_parameters())
    for k, v in sub_dict(g, 'grad/').items():
        _close(grads[k].grad, v, 1e-5, 'd' + k, gpu_tol=2e-5)


def test_adam_trajectory_through_drop_in():
    """Five steps of the reference's train step (Model_Trainer.py:71-87) on the drop-in module."""
    g = _golden('g4_stcgnn_small')
    model = _small_model(g)
    model.load_state_dict(sub_dict(g, 'sd/'))
    opt = torch.optim.Adam(model.parameters(), lr=2e-3, weight_decay=1e-4)
    losses = []
    for _ in range(5):
        loss = O.combo_loss(model(X_seq=g['X'], As=g['As'], Ac=g['Ac']), g['Y'])
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert torch.allclose(torch.tensor(losses, dtype=torch.float64), g['adam_losses'].cpu(), rtol=0, atol=2e-5), losses


def test_sf_shape_fixed_graphs_through_modules(monkeypatch):
    """g5: the reference's encoder-decoder-head at the SF shape (B = 32, T = 9, N = 100, C = 5, h = 16) on the dense graphs its own MGP_Gen
    produced, handed in as differentiable leaves: prediction, every parameter gradient, dGs and dGc.  Runs on the small-graph cell kernels
    with LEARNED graphs (asserted): dGs / dGc come from the stacked products of stc_hip/small.py over what the cell launches leave."""
    small_calls = []
    real_small = ops.stc_small_graph
    monkeypatch.setattr(ops, 'stc_small_graph', lambda *a, **k: (small_calls.append(1), real_small(*a, **k))[1])
    g = _golden('g5_sf_shape')
    model = _small_model(g, graph_mode='csr-fixed')
    sd = sub_dict(g, 'sd/')
    assert sorted(model.state_dict().keys()) == sorted(sd.keys())      # no mix_graph_pair.* in csr-fixed mode
    model.load_state_dict(sd)
    Gs, Gc = _leaf(g['Gs']), _leaf(g['Gc'])
    yhat = model(X_seq=g['X'].float(), As=Gs, Ac=Gc)                  # a dense Gs handed in directly stays differentiable
    assert yhat.shape == (32, 3, 100, 5) and small_calls, 'the small-graph path was not taken'
    _close(yhat, g['yhat'], FWD, 'SF yhat')
    O.combo_loss(yhat, g['Y'].float()).backward()
    grads = dict(model.named_parameters())
    for k, v in sub_dict(g, 'grad/').items():
        _close(grads[k].grad, v, 1e-5, 'SF d' + k, gpu_tol=2e-5)
    _close(Gs.grad, g['dGs'], 1e-5, 'SF dGs', gpu_tol=2e-5)
    _close(Gc.grad, g['dGc'], 1e-5, 'SF dGc', gpu_tol=2e-5)


@pytest.mark.parametrize('N,C,layers,T,horizon,seed', [(12, 3, 2, 4, 2, 7), (20, 5, 1, 3, 3, 25)])
def test_learned_graphs_on_the_small_graph_kernels(dev, monkeypatch, N, C, layers, T, horizon, seed):
    """The reference's FULL model (MGP_Gen's learned dense Gs and Gc, STC_GNN.py:185-261) at hidden 16 runs its cells on the small-graph
    kernels (asserted); every gradient -- including those that reach MGP_Gen's parameters through dGs and dGc, which this path forms as
    stacked products over all cells (stc_hip/small.py) -- against the float64 oracle of the same model."""
    calls = []
    real_small = ops.stc_small_graph
    monkeypatch.setattr(ops, 'stc_small_graph', lambda *a, **k: (calls.append(1), real_small(*a, **k))[1])
    torch.manual_seed(seed)
    model = M.STCGNN(N, C, 2, 2, 1, 16, layers, horizon).to(DEV)
    X = (torch.rand(2, T, N, C) < 0.3).float()
    As, Ac, Rw = torch.rand(N, N), torch.rand(C, C), torch.randn(2, horizon, N, C)
    y = model(X_seq=X.to(DEV), As=As.to(DEV), Ac=Ac.to(DEV))
    assert calls, 'the small-graph path was not taken'
    (y * Rw.to(DEV)).sum().backward()
    got = {n: p.grad.detach().clone() for n, p in model.named_parameters()}
    monkeypatch.setattr(ops, '_SMALL', False)                       # the general path: one autograd node per cell, dGs / dGc per convolution
    model.zero_grad(set_to_none=True)
    (model(X_seq=X.to(DEV), As=As.to(DEV), Ac=Ac.to(DEV)) * Rw.to(DEV)).sum().backward()
    per_cell = {n: p.grad.detach().clone() for n, p in model.named_parameters()}
    sd = {k: v.detach().cpu().double().requires_grad_(True) for k, v in model.state_dict().items()}
    want = O.stcgnn_forward(X.double(), As.double(), Ac.double(), sd, 2, 2, 16, layers, horizon)
    (want * Rw.double()).sum().backward()
    _close(y, want.detach().float().to(DEV), FWD, 'learned small-graph yhat')
    for n in got:
        # (the draws are chosen well-conditioned: for about half of all seeds MGP_Gen's OWN fp32 backward -- torch ops on either path -- is
        # 1e-5 .. 4e-5 away from the float64 value on the 3 x 3 category graph's parameters, identically on both paths)
        _close(got[n], sd[n].grad.float().to(DEV), 1e-5, f'learned small-graph d{n}', gpu_tol=2e-5)
        if n.startswith('mix_graph_pair'):        # and against the general path, which forms dGs / dGc per convolution
            _close(got[n], per_cell[n], 5e-6, f'learned small-graph d{n} vs the per-cell path', gpu_tol=1e-5)


@pytest.mark.parametrize('N,C,K,cin', [(10, 8, 2, 1), (12, 4, 2, 16), (9, 8, 3, 4), (8, 2, 2, 1), (7, 8, 2, 1), (10, 5, 2, 1)]
                         # every C the packed kernels take (tests/shape_lattice.py): two tiles of 16 // C nodes and a ragged third, every input width
                         + [(2 * (16 // C) + 1, C, 2 + C % 2, (1, 2, 3, 4, 16)[C % 5]) for C in range(1, 17)])
def test_stc_cell_on_a_fixed_graph_packs_few_categories_into_the_fused_kernels(monkeypatch, N, C, K, cin):
    """One STC_Cell (STC_GNN.py:65-79) on a fixed sparse graph through the per-cell path: where C divides 16 (and the node count divides too) its
    FUSED kernels -- gate math in the node kernels' epilogues and prologues -- run 16 / C nodes per row tile (``ops._cell_pack``, asserted); C = 5
    and an odd node count take the composed sequence on the packed plain node kernels.  New state and every gradient against the float64 oracle."""
    B, h = 2, 16
    packs = []
    real = ops._cell_pack
    monkeypatch.setattr(ops, '_cell_pack', lambda *a: packs.append(real(*a)) or packs[-1])
    gen = torch.Generator().manual_seed(31 * N + C + K)
    Gs = torch.rand(N, N, generator=gen) * (torch.rand(N, N, generator=gen) < 0.4) / 3
    Gc = torch.softmax(torch.randn(C, C, generator=gen), -1)
    Xt, Ht = torch.randn(B, N, C, cin, generator=gen), torch.tanh(torch.randn(B, N, C, h, generator=gen))
    R = torch.randn(B, N, C, h, generator=gen)
    cell = M.STC_Cell(N, C, K, K, cin, h).to(DEV)
    sd = {k: v.detach().cpu().double().requires_grad_() for k, v in cell.state_dict().items()}
    Xd, Hd = _leaf(Xt), _leaf(Ht)
    out = cell(CsrGraph.from_dense(Gs, device=DEV) if DEV == 'cuda' else CsrGraph.from_dense(Gs), Gc.to(DEV), Xd, Hd)
    (out * R.to(DEV)).sum().backward()
    L = cin + h + (-(cin + h)) % 4
    fused = ops.kernels().cell_fused_supported       # (the CPU twin fuses at any C; the library at C in {16, 32, 64})
    expect = 1 if fused(K, K, C, L, h) else (16 // C if (16 % C == 0 and (B * N) % (16 // C) == 0 and fused(K, K, 16, L, h)) else 0)
    assert packs and set(packs) == {expect}
    if DEV == 'cuda':
        assert expect == (16 // C if (16 % C == 0 and (B * N) % (16 // C) == 0) else 0)
    X64, H64 = Xt.double().requires_grad_(), Ht.double().requires_grad_()
    want = O.stc_cell(Gs.double(), Gc.double(), X64, H64, sd['gates.W'], sd['gates.b'], sd['candi.W'], sd['candi.b'], K, K)
    (want * R.double()).sum().backward()
    _close(out, want.detach().float().to(DEV), FWD, f'packed cell Hnew C={C} K={K}')
    _close(Xd.grad, X64.grad.float().to(DEV), GRAD, f'packed cell dXt C={C} K={K}')
    _close(Hd.grad, H64.grad.float().to(DEV), GRAD, f'packed cell dHt C={C} K={K}')
    for n, p_ in cell.named_parameters():
        _close(p_.grad, sd[n].grad.float().to(DEV), GRAD, f'packed cell d{n} C={C} K={K}')


@pytest.mark.parametrize('cin', [16, 1])
def test_stc_cell_with_a_learned_category_graph_at_64_categories_and_order_3(monkeypatch, cin):
    """One STC_Cell (STC_GNN.py:65-79) at C = 64, K = 3 with a DIFFERENTIABLE category graph: its gates convolution (Ho = 32) asks the node
    backward for dT_c at the one matrix-core shape where a single launch of the generic kernel is beyond its LDS limit -- the tensor front then
    forms dT_c block by block (``HipKernels._node_bwd_dT_by_block``, asserted on the GPU).  New state and every gradient, dGc included, against
    the float64 oracle."""
    N, C, K, B, h = 5, 64, 3, 2, 16
    split = []
    if DEV == 'cuda':
        from stc_hip._lib import HipKernels
        real = HipKernels._node_bwd_dT_by_block
        monkeypatch.setattr(HipKernels, '_node_bwd_dT_by_block', lambda self, *a: split.append(a[-2][:2]) or real(self, *a))
    gen = torch.Generator().manual_seed(64 * K + cin)
    Gs = torch.rand(N, N, generator=gen) * (torch.rand(N, N, generator=gen) < 0.6) / 3
    Gc = torch.softmax(torch.randn(C, C, generator=gen), -1)
    Xt, Ht = torch.randn(B, N, C, cin, generator=gen), torch.tanh(torch.randn(B, N, C, h, generator=gen))
    R = torch.randn(B, N, C, h, generator=gen)
    cell = M.STC_Cell(N, C, K, K, cin, h).to(DEV)
    sd = {k: v.detach().cpu().double().requires_grad_() for k, v in cell.state_dict().items()}
    Xd, Hd, Gcd = _leaf(Xt), _leaf(Ht), _leaf(Gc)
    out = cell(CsrGraph.from_dense(Gs, device=DEV) if DEV == 'cuda' else CsrGraph.from_dense(Gs), Gcd, Xd, Hd)
    (out * R.to(DEV)).sum().backward()
    if DEV == 'cuda':
        assert split == [(K, K)], split                              # the gates convolution alone: the candidate's (Ho = 16) fits one launch
    X64, H64, Gc64 = Xt.double().requires_grad_(), Ht.double().requires_grad_(), Gc.double().requires_grad_()
    want = O.stc_cell(Gs.double(), Gc64, X64, H64, sd['gates.W'], sd['gates.b'], sd['candi.W'], sd['candi.b'], K, K)
    (want * R.double()).sum().backward()
    _close(out, want.detach().float().to(DEV), FWD, f'C=64 K=3 learned Gc Hnew cin={cin}')
    for name, got, ref in (('dXt', Xd.grad, X64.grad), ('dHt', Hd.grad, H64.grad), ('dGc', Gcd.grad, Gc64.grad)):
        _close(got, ref.float().to(DEV), GRAD, f'C=64 K=3 learned Gc {name} cin={cin}')
    for n, p_ in cell.named_parameters():
        _close(p_.grad, sd[n].grad.float().to(DEV), GRAD, f'C=64 K=3 learned Gc d{n} cin={cin}')


@pytest.mark.parametrize('N,C,K,layers,T,horizon,seed', [(12, 3, 2, 2, 4, 2, 7), (20, 5, 3, 1, 3, 3, 3), (10, 8, 2, 2, 3, 2, 13), (9, 4, 3, 1, 3, 2, 3)])
def test_learned_graphs_on_the_general_path_with_packed_node_kernels(dev, monkeypatch, N, C, K, layers, T, horizon, seed):
    """The reference's FULL model with learned graphs on the GENERAL per-cell path (what learned graphs beyond the few-category cell kernels'
    reach take, and every learned graph at Chebyshev order 3 -- ``Main.py -K 3``): its node kernels run few categories as packed tiles on the
    matrix cores (``ops._node_pack``, asserted) and ``stc_mix_dt_f32`` forms dT_c.  Prediction and every gradient against the float64
    oracle of the same model (STC_GNN.py:185-261)."""
    packs = []
    real = ops._node_pack
    monkeypatch.setattr(ops, '_node_pack', lambda *a: packs.append(real(*a)) or packs[-1])
    monkeypatch.setattr(ops, '_SMALL', False)
    torch.manual_seed(seed)
    model = M.STCGNN(N, C, K, K, 1, 16, layers, horizon).to(DEV)
    X = (torch.rand(2, T, N, C) < 0.3).float()
    As, Ac, Rw = torch.rand(N, N), torch.rand(C, C), torch.randn(2, horizon, N, C)
    y = model(X_seq=X.to(DEV), As=As.to(DEV), Ac=Ac.to(DEV))
    (y * Rw.to(DEV)).sum().backward()
    assert packs and set(packs) == {16 // C if (2 * N) % (16 // C) == 0 else 1}      # (small node counts: no split launch for a remainder)
    sd = {k: v.detach().cpu().double().requires_grad_(True) for k, v in model.state_dict().items()}
    want = O.stcgnn_forward(X.double(), As.double(), Ac.double(), sd, K, K, 16, layers, horizon)
    (want * Rw.double()).sum().backward()
    # the reference's own arithmetic (the oracle in float32) against float64: at order 3 the learned graphs' T_2 = 2 G^2 - I amplifies rounding, and
    # fp32 itself is 1e-4 .. 1e-3 away on MGP_Gen's parameters for most draws -- the bound is 10x that noise where it exceeds the flat one
    sd32 = {k: v.detach().cpu().float().requires_grad_(True) for k, v in model.state_dict().items()}
    (O.stcgnn_forward(X, As, Ac, sd32, K, K, 16, layers, horizon) * Rw).sum().backward()
    _close(y, want.detach().float().to(DEV), FWD, f'learned general-path yhat C={C} K={K}')
    for n, p in model.named_parameters():
        noise = rel_err(sd32[n].grad, sd[n].grad)
        _close(p.grad, sd[n].grad.float().to(DEV), max(1e-5, 10 * noise), f'learned general-path d{n} C={C} K={K}', gpu_tol=max(2e-5, 10 * noise))


def test_learned_graph_gradients_when_a_sets_cells_are_unevenly_spaced(monkeypatch):
    """``small._graph_gradients`` selects a parameter set's cells by (first, step) inside their width group; a schedule where they are NOT
    evenly spaced (STCGNN never builds one) takes the gathering fallback -- with every product's partials in the shared buffers.  Learned dense
    Gs and Gc, two parameter sets interleaved 0, 1, 0, 0, 1: gradients of both graphs and of every parameter against the float64 oracle."""
    from stc_hip.graph import dense_operand
    N, C, B, h = 23, 5, 3, 16
    g = torch.Generator().manual_seed(7)
    base = {'Gs': torch.rand(N, N, generator=g) / N, 'Gc': torch.rand(C, C, generator=g) / C,
            'X': torch.randn(B, N, C, h, generator=g), 'H': torch.tanh(torch.randn(B, N, C, h, generator=g)), 'R': torch.randn(B, N, C, h, generator=g)}
    for s_id in (0, 1):
        base[f'Wg{s_id}'], base[f'Wc{s_id}'] = torch.randn(4 * 2 * h, 2 * h, generator=g) * 0.1, torch.randn(4 * 2 * h, h, generator=g) * 0.1
        base[f'bg{s_id}'], base[f'bc{s_id}'] = torch.randn(2 * h, generator=g) * 0.1, torch.randn(h, generator=g) * 0.1
    schedule = [(0, ('ext', 0), ('ext', 1)), (1, ('cell', 0), ('ext', 1)), (0, ('cell', 1), ('cell', 0)), (0, ('cell', 2), ('cell', 1)), (1, ('cell', 3), ('cell', 2))]

    def run(small):
        monkeypatch.setattr(ops, '_SMALL', small)
        # (the external tensors and the weights of the loss are data: the executor refuses an external tensor that requires grad)
        t = {k: (v.clone().to(DEV) if k in ('X', 'H', 'R') else _leaf(v)) for k, v in base.items()}
        op, Tc = dense_operand(t['Gs']), ops.cheby_dense(t['Gc'], 2)
        stacks = [(t[f'Wg{s}'], t[f'bg{s}'], t[f'Wc{s}'], t[f'bc{s}']) for s in (0, 1)]
        if small:
            assert ops.cell_graph_supported(op, Tc, 2, C, h, [h])
        out = ops.stc_cell_graph(op, Tc, 2, schedule, [4], [t['X'], t['H']], stacks)[0]
        (out * t['R']).sum().backward()
        return out.detach(), {k: v.grad for k, v in t.items() if k not in ('X', 'H', 'R')}

    calls = []
    from stc_hip import small as small_mod
    real = small_mod._graph_gradients
    monkeypatch.setattr(small_mod, '_graph_gradients', lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    out_s, grads_s = run(True)
    assert calls, 'the few-category executor was not taken'
    # the float64 oracle of the same schedule (the reference's cell, STC_GNN.py:65-79, dense Gs)
    w = {k: v.double().requires_grad_() for k, v in base.items()}
    ext, states = [w['X'], w['H']], []
    for s_id, x, hs in schedule:
        src = lambda ref: ext[ref[1]] if ref[0] == 'ext' else states[ref[1]]
        states.append(O.stc_cell(w['Gs'], w['Gc'], src(x), src(hs), w[f'Wg{s_id}'], w[f'bg{s_id}'], w[f'Wc{s_id}'], w[f'bc{s_id}'], 2, 2))
    (states[4] * w['R']).sum().backward()
    _close(out_s, states[4].detach().float().to(DEV), FWD, 'uneven schedule: state')
    for k in grads_s:
        _close(grads_s[k], w[k].grad.float().to(DEV), 1e-5, f'uneven schedule: d{k}', gpu_tol=2e-5)


@pytest.mark.parametrize('tag,fname', [('g7', 'g7_csr_n1024'), ('g7p', 'g7_csr_n1024_perm')])
@pytest.mark.parametrize('form', ['CsrGraph', 'torch_sparse'])
def test_csr_fixed_graph_equals_dense_reference(tag, fname, form):
    """A sparse Gs through the CSR path equals the reference fed the same matrix densely (K=3)."""
    g = _golden(fname)
    s = {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in synth_inputs(tag).items()}
    graph = CsrGraph.from_dense(s['Gs']) if form == 'CsrGraph' else s['Gs'].cpu().to_sparse_coo()
    cell = M.STC_Cell(s['N'], s['C'], s['K'], s['K'], s['cin'], s['h']).to(DEV)
    cell.load_state_dict({'gates.W': s['gates_W'], 'gates.b': s['gates_b'], 'candi.W': s['candi_W'], 'candi.b': s['candi_b']})
    Xt, Ht = _leaf(s['Xt']), _leaf(s['Ht'])
    out = cell(graph, s['Gc'], Xt, Ht)
    rows = g['rows']
    _close(out[:, rows], g['Hout'], FWD, 'Ht rows')
    (out * s['R']).sum().backward()
    _close(Xt.grad[:, rows], g['dXt'], GRAD, 'dXt rows')
    _close(Ht.grad[:, rows], g['dHt'], GRAD, 'dHt rows')
    _close(cell.gates.W.grad, g['d_gates_W'], 2e-5, 'dgates.W', gpu_tol=2e-5)
    _close(cell.candi.W.grad, g['d_candi_W'], 2e-5, 'dcandi.W', gpu_tol=2e-5)
    _close(cell.gates.b.grad, g['d_gates_b'], 2e-5, 'dgates.b', gpu_tol=2e-5)


def test_large_n10000_against_dense_reference_rows():
    """N = 10 000, C = 32, h = 16 (config 4 width): CSR path vs 128 rows of the dense reference."""
    g = _golden('g8_large_n10000')
    s = synth_inputs('g8')
    graph = CsrGraph.from_dense(s.pop('Gs'))
    s = {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in s.items()}
    cell = M.STC_Cell(s['N'], s['C'], s['K'], s['K'], s['cin'], s['h']).to(DEV)
    cell.load_state_dict({'gates.W': s['gates_W'], 'gates.b': s['gates_b'], 'candi.W': s['candi_W'], 'candi.b': s['candi_b']})
    with torch.no_grad():
        out = cell(graph, s['Gc'], s['Xt'], s['Ht'])
    _close(out[:, g['rows']], g['Hout'], FWD, 'Ht rows N=10000')


def test_large_n10000_gradients_against_dense_reference_rows():
    """g8b: the same cell WITH backward -- sampled rows of dXt / dHt and the full parameter gradients of the dense reference."""
    g = _golden('g8b_large_n10000_grads')
    s = synth_inputs('g8')
    graph = CsrGraph.from_dense(s.pop('Gs'))
    s = {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in s.items()}
    cell = M.STC_Cell(s['N'], s['C'], s['K'], s['K'], s['cin'], s['h']).to(DEV)
    cell.load_state_dict({'gates.W': s['gates_W'], 'gates.b': s['gates_b'], 'candi.W': s['candi_W'], 'candi.b': s['candi_b']})
    Xt, Ht = _leaf(s['Xt']), _leaf(s['Ht'])
    out = cell(graph, s['Gc'], Xt, Ht)
    rows = g['rows']
    _close(out[:, rows], g['Hout'], FWD, 'Ht rows N=10000 (g8b)')
    (out * s['R']).sum().backward()
    _close(Xt.grad[:, rows], g['dXt'], GRAD, 'dXt rows N=10000')
    _close(Ht.grad[:, rows], g['dHt'], GRAD, 'dHt rows N=10000')
    for name, p in (('d_gates_W', cell.gates.W), ('d_gates_b', cell.gates.b), ('d_candi_W', cell.candi.W), ('d_candi_b', cell.candi.b)):
        _close(p.grad, g[name], 2e-5, name + ' N=10000', gpu_tol=2e-5)


@pytest.mark.parametrize('K', [2, 3])
def test_bdg_dif_at_baseline_configuration_2(K):
    """BASELINE configuration 2 at its own shape: ONE BDG_Dif layer (STC_GNN.py:31-47), B = 32, N = 200, C = 8, L = 32, Ho = 32, dense
    learned (differentiable) Gs and Gc, against the oracle's op-for-op restatement of the reference (``oracle.bdg_dif``: dense einsum,
    matrix-side cheby_poly, concat + projection) -- forward and dX, dW, db, dGs, dGc."""
    B, N, C, L, Ho = 32, 200, 8, 32, 32
    gen = torch.Generator().manual_seed(200 + K)
    X = torch.randn(B, N, C, L, generator=gen)
    Gs = torch.softmax(torch.randn(N, N, generator=gen), -1)                 # row-stochastic, dense, NON-symmetric (as MGP_Gen's output)
    Gc = torch.softmax(torch.randn(C, C, generator=gen), -1)
    W = torch.randn(K * K * L, Ho, generator=gen) * (2.0 / (K * K * L + Ho)) ** 0.5
    bias = torch.randn(Ho, generator=gen) * 0.1
    R = torch.randn(B, N, C, Ho, generator=gen)
    # the oracle in float64 (it is dtype-generic): dGc and dW are sums over B*N*L = 204 800 .. 1.6 M products, where an fp32 CPU sum is
    # itself 1e-5 away from the exact value -- the more exact side of the comparison must be the reference side
    want_in = [t.double().requires_grad_() for t in (X, Gs, Gc, W, bias)]
    want = O.bdg_dif(want_in[0], want_in[1], want_in[2], want_in[3], want_in[4], K, K)
    (want * R.double()).sum().backward()
    layer = M.BDG_Dif(K, K, L, Ho).to(DEV)
    layer.load_state_dict({'W': W, 'b': bias})
    Xd, Gsd, Gcd = _leaf(X), _leaf(Gs), _leaf(Gc)
    got = layer(Xd, Gsd, Gcd)
    _close(got, want.detach().float().to(DEV), FWD, f'cfg2 K={K} Y')
    (got * R.to(DEV)).sum().backward()
    for name, t, w in (('dX', Xd.grad, want_in[0].grad), ('dGs', Gsd.grad, want_in[1].grad), ('dGc', Gcd.grad, want_in[2].grad),
                       ('dW', layer.W.grad, want_in[3].grad), ('db', layer.b.grad, want_in[4].grad)):
        _close(t, w.float().to(DEV), GRAD, f'cfg2 K={K} {name}')


@pytest.mark.parametrize('C,N,K,L,Ho', [(8, 50, 2, 32, 32), (4, 36, 3, 32, 16), (2, 24, 2, 20, 32), (8, 25, 2, 32, 32), (5, 20, 2, 32, 32), (5, 100, 3, 20, 32),
                                        (7, 13, 2, 32, 16), (12, 9, 3, 32, 32), (16, 10, 2, 20, 16)]
                         # every C the packed kernels take (tests/shape_lattice.py): two tiles of 16 // C nodes and a ragged third
                         + [(C, 2 * (16 // C) + 1, 2 + C % 2, (32, 20)[(C // 2) % 2], (32, 16)[(C // 4) % 2]) for C in range(1, 17)])
def test_bdg_dif_packs_few_categories_into_matrix_core_tiles(monkeypatch, C, N, K, L, Ho):
    """Few categories (C <= 16): floor(16 / C) consecutive nodes run as ONE node of up to 16 categories with a block-diagonal category graph
    on the matrix-core node kernels (``ops._node_pack``; reference STC_GNN.py:38-45 is node-local), dT_c from ``ops._mix_grad``.  Against the
    float64 oracle, and equal (to rounding) to the unpacked launches; an odd row count (N = 25, one sample): the last node runs alone."""
    B = 1 if N == 25 else 3
    gen = torch.Generator().manual_seed(C * 100 + K)
    X = torch.randn(B, N, C, L, generator=gen)
    Lw = L if L == 32 else 17
    X[..., Lw:] = 0                                                           # (L = 20: rows padded to 16 bytes, W keeps 17 rows per block)
    Gs = torch.softmax(torch.randn(N, N, generator=gen), -1)
    Gc = torch.softmax(torch.randn(C, C, generator=gen), -1)
    W = torch.randn(K * K * Lw, Ho, generator=gen) * (2.0 / (K * K * Lw + Ho)) ** 0.5
    bias = torch.randn(Ho, generator=gen) * 0.1
    R = torch.randn(B, N, C, Ho, generator=gen)
    packs = []
    real = ops._node_pack
    monkeypatch.setattr(ops, '_node_pack', lambda *a: packs.append(real(*a)) or packs[-1])
    monkeypatch.setattr(ops, '_PACK_SPLIT_ROWS', 0)                   # (small shapes here: split a remainder off at any size)
    want_in = [t.double().requires_grad_() for t in (X[..., :Lw], Gs, Gc, W, bias)]
    want = O.bdg_dif(*want_in, K, K)
    (want * R.double()).sum().backward()

    def run():
        layer = M.BDG_Dif(K, K, Lw, Ho).to(DEV)
        layer.load_state_dict({'W': W, 'b': bias})
        Xd, Gsd, Gcd = _leaf(X), _leaf(Gs), _leaf(Gc)
        Y = layer(Xd, Gsd, Gcd, _pad=L - Lw)
        (Y * R.to(DEV)).sum().backward()
        return Y.detach(), Xd.grad[..., :Lw], Gsd.grad, Gcd.grad, layer.W.grad, layer.b.grad

    got = run()
    assert packs and set(packs) == {16 // C}                         # (C = 5: three nodes = 15 rows per tile; an odd row count: the last node alone)
    names = ('Y', 'dX', 'dGs', 'dGc', 'dW', 'db')
    for name, t, w in zip(names, got, (want.detach(), *(v.grad for v in want_in))):
        _close(t, w.float().to(DEV), FWD if name == 'Y' else GRAD, f'packed C={C} K={K} {name}')
    monkeypatch.setattr(ops, '_NODE_PACK', False)
    plain = run()
    for name, a, b in zip(names, got, plain):
        assert rel_err(a, b) < 2e-6, f'packed vs unpacked {name}: {rel_err(a, b):.2e}'


def test_large_n10000_order_3_against_dense_reference_rows():
    """g8c: one STC_Cell at N = 10 000, C = 32, h = 16, Chebyshev order K = 3 (BASELINE configuration 4) against the dense reference
    (STC_GNN.py:24-29, 65-79) -- new state, dXt, dHt on 256 sampled rows and the full parameter gradients."""
    g = _golden('g8c_large_n10000_k3')
    s = synth_inputs('g8c')
    graph = CsrGraph.from_dense(s.pop('Gs'))
    s = {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in s.items()}
    cell = M.STC_Cell(s['N'], s['C'], 3, 3, s['cin'], s['h']).to(DEV)
    cell.load_state_dict({'gates.W': s['gates_W'], 'gates.b': s['gates_b'], 'candi.W': s['candi_W'], 'candi.b': s['candi_b']})
    Xt, Ht = _leaf(s['Xt']), _leaf(s['Ht'])
    out = cell(graph, s['Gc'], Xt, Ht)
    rows = g['rows']
    _close(out[:, rows], g['Hout'], FWD, 'Ht rows N=10000 K=3 (g8c)')
    (out * s['R']).sum().backward()
    _close(Xt.grad[:, rows], g['dXt'], GRAD, 'dXt rows N=10000 K=3')
    _close(Ht.grad[:, rows], g['dHt'], GRAD, 'dHt rows N=10000 K=3')
    for name, p in (('d_gates_W', cell.gates.W), ('d_gates_b', cell.gates.b), ('d_candi_W', cell.candi.W), ('d_candi_b', cell.candi.b)):
        _close(p.grad, g[name], 2e-5, name + ' N=10000 K=3', gpu_tol=2e-5)


def test_large_n10000_order_3_planar_cells_against_dense_reference_rows():
    """g8c through the path the bench takes at order 3: the cell as a one-cell schedule of ``ops.stc_cell_graph``, i.e. the order-3 PLANAR
    kernels (three Chebyshev planes per side, stc_cell_*_planar_k_f32) at N = 10 000 -- new state on 256 rows and every parameter gradient
    of the dense reference; then two chained cells (the second one reads the first one's state as X and as H, so the state's gradient is
    assembled from its consumers' planes by the Clenshaw sums) against the oracle's sparse restatement."""
    g = _golden('g8c_large_n10000_k3')
    s = synth_inputs('g8c')
    graph = CsrGraph.from_dense(s.pop('Gs'))
    sc = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in s.items()}
    s = {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in s.items()}
    from stc_hip.graph import csr_operand
    op = csr_operand(graph, torch.device(DEV))
    Tc = ops.cheby_dense(s['Gc'], 3)
    assert ops.cell_graph_supported(op, Tc, 3, s['C'], s['h'], [s['cin']]), 'order-3 planar cells are not available for this shape'
    p = [_leaf(s[k]) for k in ('gates_W', 'gates_b', 'candi_W', 'candi_b')]
    out = ops.stc_cell_graph(op, Tc, 3, [(0, ('ext', 0), ('ext', 1))], [0], [s['Xt'], s['Ht']], [tuple(p)])[0]
    rows = g['rows']
    _close(out[:, rows], g['Hout'], FWD, 'planar-K Ht rows N=10000 K=3 (g8c)')
    (out * s['R']).sum().backward()
    for t, name in zip(p, ('d_gates_W', 'd_gates_b', 'd_candi_W', 'd_candi_b')):
        _close(t.grad, g[name], 2e-5, 'planar-K ' + name + ' N=10000 K=3', gpu_tol=2e-5)
    # two chained cells: state gradients through the Clenshaw sums, against the oracle (float64: sums over 320 000 rows)
    p2 = [_leaf(s[k]) for k in ('gates_W', 'gates_b', 'candi_W', 'candi_b')]
    out2 = ops.stc_cell_graph(op, Tc, 3, [(0, ('ext', 0), ('ext', 1)), (0, ('cell', 0), ('cell', 0))], [1], [s['Xt'], s['Ht']], [tuple(p2)])[0]
    (out2 * s['R']).sum().backward()
    GsT = graph_dense_T_csr(sc, graph)
    po = [sc[k].double().requires_grad_() for k in ('gates_W', 'gates_b', 'candi_W', 'candi_b')]
    s0 = O.stc_cell(GsT, sc['Gc'].double(), sc['Xt'].double(), sc['Ht'].double(), *po, 3, 3, conv=O.bdg_dif_sparse)
    s1 = O.stc_cell(GsT, sc['Gc'].double(), s0, s0, *po, 3, 3, conv=O.bdg_dif_sparse)
    (s1 * sc['R'].double()).sum().backward()
    _close(out2[:, rows], s1.detach()[:, rows.cpu()].float().to(DEV), FWD, 'two chained planar-K cells: Ht rows')
    for t, w, name in zip(p2, po, ('d_gates_W', 'd_gates_b', 'd_candi_W', 'd_candi_b')):
        _close(t.grad, w.grad.float().to(DEV), 2e-5, 'two chained planar-K cells: ' + name, gpu_tol=2e-5)


def graph_dense_T_csr(s, graph):
    h = graph._host
    return torch.sparse_csr_tensor(torch.from_numpy(h['fwd_rowptr']).long(), torch.from_numpy(h['fwd_colidx']).long(),
                                   torch.from_numpy(h['fwd_val']).double(), size=(graph.n, graph.n))


@pytest.mark.parametrize('name,C,K', [('g11_bench_c32', 32, 2), ('g12_bench_c64', 64, 2), ('g13_bench_c32_k3', 32, 3), ('g14_sf_shape', 5, 2), ('g15_sf_shape_k3', 5, 3)])
def test_bench_path_against_reference_goldens(monkeypatch, name, C, K):
    """The path bench.py runs -- csr-fixed STCGNN at C in {32, 64}, hidden 16, encoder + decoder as ONE cell-graph node on the
    planar / split-operand matrix-core kernels -- against goldens the REFERENCE generated at exactly these widths
    (STC_GNN.py:185-207 after MGP_Gen, Model_Trainer.py:14-23): prediction, ComboLoss, every parameter gradient, 1e-5.
    g14: the SF-incidents shape (N = 100, C = 5, T = 9 + 3; ``bench.py --preset sf``), which runs on the small-graph cell kernels
    (one launch per cell step: stc_cell_small_fwd/bwd_f32) -- asserted taken; g15: the same shape at Chebyshev order 3 (T_2(S) as a second graph)."""
    g = _golden(name)
    s = bench_path_inputs(C, K, **(SF_SHAPE if name in ('g14_sf_shape', 'g15_sf_shape_k3') else {}))
    small_calls = []
    real_small = ops.stc_small_graph
    monkeypatch.setattr(ops, 'stc_small_graph', lambda *a, **k: (small_calls.append(1), real_small(*a, **k))[1])
    model = _small_model(g, graph_mode='csr-fixed')
    sd = sub_dict(g, 'sd/')
    assert sorted(model.state_dict().keys()) == sorted(sd.keys())
    model.load_state_dict(sd)
    graph = CsrGraph.from_dense(s['Gs'])
    calls = []
    real = ops.stc_cell_graph
    monkeypatch.setattr(ops, 'stc_cell_graph', lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    yhat = model(X_seq=s['X'].to(DEV), As=graph, Ac=s['Gc'].to(DEV))
    assert calls, 'the cell-graph path (the one the bench runs) was not taken'
    assert bool(small_calls) == (name in ('g14_sf_shape', 'g15_sf_shape_k3'))
    _close(yhat, g['yhat'], FWD, f'{name} yhat')
    loss = O.combo_loss(yhat, s['Y'].to(DEV))
    assert abs(float(loss.detach()) - float(g['loss'])) < 5e-6
    loss.backward()
    grads = dict(model.named_parameters())
    for k, v in sub_dict(g, 'grad/').items():
        _close(grads[k].grad, v, GRAD, f'{name} d{k}')


def test_internal_node_reordering_is_invisible():
    """A graph handed over in a random node order is renumbered internally (reverse Cuthill-McKee); predictions and
    gradients are those of the un-reordered run (only the summation order inside a row changes)."""
    graph = CsrGraph.queen_grid(12, 11, permute_seed=4)
    cand, order = graph.with_locality()
    assert order is not None and cand.fetches_per_row[0] * 1.25 <= graph.fetches_per_row[0]
    assert CsrGraph.queen_grid(12, 11).with_locality()[1] is None            # already banded: left alone
    torch.manual_seed(3)
    N, C = graph.n, 4
    kw = dict(num_nodes=N, num_categories=C, Ks=2, Kc=2, input_dim=1, hidden_dim=8, num_layers=2, out_horizon=2, graph_mode='csr-fixed')
    plain = M.STCGNN(**kw, reorder_nodes=False).to(DEV)
    smart = M.STCGNN(**kw).to(DEV)
    smart.load_state_dict(plain.state_dict())
    X = (torch.rand(2, 3, N, C) < 0.3).float().to(DEV)
    Gc = torch.softmax(torch.randn(C, C), -1).to(DEV)
    R = torch.randn(2, 2, N, C).to(DEV)
    ya, yb = plain(X_seq=X, As=graph, Ac=Gc), smart(X_seq=X, As=graph, Ac=Gc)
    _close(yb, ya, FWD, 'reordered yhat')
    sparse = graph.to_dense().to_sparse_coo()                     # a torch sparse graph is renumbered internally as well
    yc = smart(X_seq=X, As=sparse, Ac=Gc)
    assert sparse._stc_csr.with_locality()[1] is not None
    _close(yc, ya, FWD, 'reordered yhat (torch sparse input)')
    (ya * R).sum().backward()
    (yb * R).sum().backward()
    for (k, pa), (_, pb) in zip(plain.named_parameters(), smart.named_parameters()):
        _close(pb.grad, pa.grad, GRAD, 'reordered d' + k)


def test_shape_errors_are_python_exceptions():
    layer = M.BDG_Dif(2, 2, 5, 4).to(DEV)
    t = lambda *s: torch.randn(*s, device=DEV)
    with pytest.raises(ValueError):
        layer(t(2, 12, 3), t(12, 12), t(3, 3))                      # rank
    with pytest.raises(ValueError):
        layer(t(2, 12, 3, 5), t(11, 11), t(3, 3))                   # node count
    with pytest.raises(ValueError):
        layer(t(2, 12, 3, 6), t(12, 12), t(3, 3))                   # feature width vs W
    cell = M.STC_Cell(12, 3, 2, 2, 1, 4).to(DEV)
    with pytest.raises(AssertionError):
        cell(t(12, 12), t(3, 3), t(2, 12, 3), t(2, 12, 3, 4))
    with pytest.raises(AssertionError):
        M.STCGNN(12, 3, 2, 2, 1, 4, 2, 2).to(DEV)(t(2, 4, 12), t(12, 12), t(3, 3))
    with pytest.raises(ValueError):
        M.STCGNN(12, 3, 2, 2, 1, 4, 2, 2, graph_mode='nope')


def test_factorised_mixed_fusion_option(dev):
    """rank-r MixedFusion.  (1) it IS the dense layer with weight U V^T; (2) a learned-graph model with it
    runs forward/backward through the kernels; (3) n = 1000 is affordable (the dense form: 2 x 10^12 parameters)."""
    torch.manual_seed(5)
    n, r = 6, 3
    fact, dense = M.MixedFusion(n, rank=r), M.MixedFusion(n)
    with torch.no_grad():
        for name in ('lin_A', 'lin_P'):
            getattr(dense, name).weight.copy_(getattr(fact, name).dense_weight())
            getattr(dense, name).bias.copy_(getattr(fact, name).bias)
    A, P = torch.rand(n, n), torch.softmax(torch.randn(n, n), -1)
    assert float((fact(A, P) - dense(A, P)).abs().max()) < 1e-6
    N, C = 40, 3
    model = M.STCGNN(N, C, 2, 2, 1, 4, 1, 2, fusion_rank=4).to(DEV)
    assert not any(p.numel() > 2 * N * N * 4 + N * N for p in model.parameters())           # no N^2 x N^2 weight anywhere
    X = (torch.rand(2, 3, N, C) < 0.3).float().to(DEV)
    As, Ac = (torch.rand(N, N) < 0.2).float().to(DEV), torch.rand(C, C).to(DEV)
    out = model(X_seq=X, As=As, Ac=Ac)
    out.sum().backward()
    assert out.shape == (2, 2, N, C) and all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())
    if DEV == 'cpu':
        big = M.MixedFusion(1000, rank=8)
        assert sum(p.numel() for p in big.parameters()) == 2 * (2 * 10 ** 6 * 8 + 10 ** 6)


@pytest.mark.parametrize('small', [False, True], ids=['wide', 'small'])
@pytest.mark.parametrize('layers,T,horizon,cin,K', [(2, 4, 3, 1, 2), (1, 3, 2, 1, 2), (3, 2, 2, 4, 2), (2, 3, 2, 1, 3), (3, 2, 2, 4, 3)])
def test_cell_graph_equals_the_per_cell_path(dev, monkeypatch, layers, T, horizon, cin, K, small, one_launch_bwd=True):
    """Encoder + decoder as one autograd node (no concat / gradient-accumulation passes between the cells) vs one node per
    cell: same prediction, same parameter gradients.  Hidden 16; 32 categories on the GPU (matrix-core shapes).  K = 3: the
    order-3 planar cells (three Chebyshev planes per side, Clenshaw state gradients) against the per-cell slab form.
    ``small``: 5 categories -- the small-graph executor (stc_hip/small.py: one launch per cell step, per-sample parameter-gradient
    partials) against the same per-cell path; at K = 3 with T_2(S) = 2 S^2 - I as a second CSR graph (round 6)."""
    monkeypatch.setattr(ops, '_SMALL', small)
    taken = []
    real_small = ops.stc_small_graph
    monkeypatch.setattr(ops, 'stc_small_graph', lambda *a, **k: (taken.append(1), real_small(*a, **k))[1])
    C = 5 if (small or DEV == 'cpu') else 32
    Hh, Ww, h, B = 5, 6, 16, 2
    if not one_launch_bwd:          # the two-launch backward is what C = 64 runs (the one-launch kernel is built for C = 32): force it at C = 32
        monkeypatch.setattr(type(ops.kernels()), 'cell_bwd_planar_supported', lambda self, Cc, hh: False)
    torch.manual_seed(layers * 10 + T)
    graph = CsrGraph.queen_grid(Hh, Ww, normalize=True)
    model = M.STCGNN(Hh * Ww, C, K, K, cin, h, layers, horizon, graph_mode='csr-fixed').to(DEV)
    if cin != 1:                                                   # the head maps back to input_dim; keep it scalar for the loss below
        model._head = lambda Hs: torch.sigmoid(Hs.sum(-1))
    Gc = torch.softmax(torch.randn(C, C), -1).to(DEV)
    X = torch.rand(B, T, Hh * Ww, C, cin).to(DEV)
    Rw = torch.randn(B, horizon, Hh * Ww, C).to(DEV)
    calls = []
    real = ops.stc_cell_graph
    monkeypatch.setattr(ops, 'stc_cell_graph', lambda *a, **k: (calls.append(1), real(*a, **k))[1])

    def run(flag):
        monkeypatch.setattr(ops, '_CELL_GRAPH', flag)
        model.zero_grad(set_to_none=True)
        pair = M._graphs(graph, Gc, K, K)
        stacked = model._run_cell_graph(pair, X) if flag else None
        if stacked is None:
            assert not flag
            _, states = model.encoder._run(pair, None, X)
            step_in, outs = states[-1], []
            for _ in range(horizon):
                step_in, states = model.decoder(pair, None, step_in, states)
                outs.append(step_in)
            y = model._head(torch.stack(outs, dim=1))
        else:
            y = model._head(stacked).transpose(0, 1)
        (y * Rw).sum().backward()
        return y.detach().clone(), {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}

    y1, g1 = run(True)
    assert calls, 'the cell-graph path was not taken'
    assert bool(taken) == small
    y0, g0 = run(False)
    _close(y1, y0, 1e-6, 'cell-graph prediction vs per-cell', gpu_tol=2e-6)
    assert set(g1) == set(g0)
    for n in g0:
        # (the head's bias gradient is one long, cancelling sum over every output element, taken in (horizon, B) order on one
        # path and (B, horizon) order on the other: summation-order noise of a few 1e-6 although the predictions are identical;
        # the small-graph executor sums parameter gradients per sample first, then over the batch: 5e-6)
        head_bias = n.startswith('out_proj') and n.endswith('bias')
        _close(g1[n], g0[n], 2e-5 if head_bias else (5e-6 if small else 2e-6), f'cell-graph d{n} vs per-cell', gpu_tol=2e-5 if head_bias else 5e-6)


@pytest.mark.parametrize('planar,post_agg,K', [(True, True, 2), (False, True, 2), (False, False, 2), (True, True, 3), (False, True, 3)])
def test_cell_graph_general_schedules_match_autograd(dev, monkeypatch, planar, post_agg, K):
    """``ops.stc_cell_graph`` on schedules STCGNN never builds -- a state consumed by FOUR cells (twice as input, twice as state),
    a cell fed by the same state on both sides, external inputs of both widths -- against the same DAG composed from
    ``ops.stc_cell`` with autograd doing the bookkeeping.  Exercises the overflow paths of the state copies and of the
    gradient pieces (more consumers than the kernels take destinations / addends for)."""
    monkeypatch.setattr(ops, '_PLANAR', planar)
    monkeypatch.setattr(ops, '_POST_AGG', post_agg)
    monkeypatch.setattr(ops, '_SMALL', False)
    _general_schedule(32 if DEV == 'cuda' else 4, K)


def test_small_graph_general_schedules_match_autograd(dev, monkeypatch):
    """The same unusual schedules through the small-graph executor (one launch per cell step; gradients of a state written / added in
    place by its consumers, the both-sides-from-one-state cell through a temporary)."""
    taken = []
    real_small = ops.stc_small_graph
    monkeypatch.setattr(ops, 'stc_small_graph', lambda *a, **k: (taken.append(1), real_small(*a, **k))[1])
    _general_schedule(5, 2, tol=6e-6)
    assert taken


# The schedule of ``_general_schedule`` (tests/autograd_contract.py runs it too): parameter set 0 = the wide cell (16 + 16 columns), 1 = the narrow
# one (1 + 16); external tensors 0 = narrow input, 1 = wide input, 2 = initial state
#                   stack, Xt source,   H source
GENERAL_SCHEDULE = [(1, ('ext', 0), ('ext', 2)),      # 0: narrow cell on external input and state
                    (0, ('ext', 1), ('cell', 0)),     # 1: wide, state from 0
                    (0, ('cell', 0), ('cell', 0)),    # 2: wide, both sides from 0
                    (0, ('cell', 0), ('cell', 1)),    # 3: wide, input from 0 (its third consumer), state from 1
                    (1, ('ext', 0), ('cell', 0)),     # 4: narrow, state from 0 (fourth consumer)
                    (0, ('cell', 2), ('cell', 3)),    # 5
                    (0, ('cell', 4), ('cell', 5))]    # 6
GENERAL_OUTPUTS = [6, 3]


def _general_schedule(C, K, tol=3e-6, schedule=GENERAL_SCHEDULE, outputs=GENERAL_OUTPUTS):
    Hh, Ww, h, B = 4, 5, 16, 2
    N = Hh * Ww
    torch.manual_seed(77)
    graph = CsrGraph.queen_grid(Hh, Ww, normalize=True)
    pair = M._graphs(graph, torch.softmax(torch.randn(C, C), -1).to(DEV), K, K)
    wide = M.STC_Cell(N, C, K, K, h, h).to(DEV)               # 16 + 16 columns
    narrow = M.STC_Cell(N, C, K, K, 1, h).to(DEV)             # 1 + 16 columns
    x0 = torch.rand(B, N, C, 1).to(DEV)
    xw = torch.rand(B, N, C, h).to(DEV)
    h0 = torch.rand(B, N, C, h).to(DEV)
    cells = (wide, narrow)
    stacks = [(c.gates.W, c.gates.b, c.candi.W, c.candi.b) for c in cells]
    Rw = torch.randn(len(outputs), B, N, C, h).to(DEV)

    def grads():
        g = {}
        for i, c in enumerate(cells):
            for n, p in c.named_parameters():
                g[f'{i}.{n}'] = p.grad.detach().clone()
                p.grad = None
        return g

    got = ops.stc_cell_graph(pair.spatial, pair.Tc, K, schedule, outputs, [x0, xw, h0], stacks)
    (got * Rw).sum().backward()
    g1 = grads()
    ext = [x0, xw, h0]
    state = []
    for s_id, xs, hs in schedule:
        src = lambda t: ext[t[1]] if t[0] == 'ext' else state[t[1]]
        state.append(cells[s_id](pair, None, src(xs), src(hs)))
    want = torch.stack([state[j] for j in outputs])
    (want * Rw).sum().backward()
    g0 = grads()
    _close(got, want, 2e-6, 'general schedule: states', gpu_tol=3e-6)
    for n in g0:
        _close(g1[n], g0[n], tol, f'general schedule: d{n}', gpu_tol=6e-6)


@pytest.mark.parametrize('planar,post_agg,K,two_launch', [(True, True, 2, False), (True, True, 2, True), (False, True, 2, False), (False, False, 2, False),
                                                          (True, True, 3, False), (False, True, 3, False)])
def test_cell_graph_fan_out_matches_autograd(dev, monkeypatch, planar, post_agg, K, two_launch):
    """``FANOUT_SCHEDULE`` (tests/launch_trace.py): ONE state consumed by eight cells, seven times as input and once as state, every consumer an
    output -- the state's record holds more planes than the state-gradient launches take addends or gather operands for, on every list: 15
    direct + 8 aggregated planes at order 2 with the two-launch backward, (8, 8, 8) at order 3.  Against the composition from ``ops.stc_cell``,
    at the tolerances of ``test_cell_graph_general_schedules_match_autograd``."""
    monkeypatch.setattr(ops, '_PLANAR', planar)
    monkeypatch.setattr(ops, '_POST_AGG', post_agg)
    monkeypatch.setattr(ops, '_SMALL', False)
    if two_launch:
        monkeypatch.setattr(type(ops.kernels()), 'cell_bwd_planar_supported', lambda self, Cc, hh: False)
    _general_schedule(32 if DEV == 'cuda' else 4, K, schedule=FANOUT_SCHEDULE, outputs=FANOUT_OUTPUTS)


def test_cell_graph_nine_order3_consumers(dev, monkeypatch):
    """One consumer more: nine planes per list at order 3, more first-ring planes than ``spmm_sum`` takes addends -- pre-summed like the
    other lists (without the pre-sum the launch is refused: ``StcError``).  Two-ring plans off: the sums go through ``spmm_sum``."""
    monkeypatch.setattr(ops, '_SMALL', False)
    monkeypatch.setattr(ops, '_RING2', False)
    _general_schedule(32 if DEV == 'cuda' else 4, 3, schedule=FANOUT_SCHEDULE + [(0, ('cell', 0), ('ext', 2))], outputs=FANOUT_OUTPUTS + [9])


@pytest.mark.parametrize('small', [False, True], ids=['wide', 'small'])
def test_cell_graph_output_stack_is_guarded_against_in_place_edits(dev, monkeypatch, small):
    """The states saved for backward alias the returned stack's storage (no copy); an in-place edit of the stack between
    forward and backward is reported instead of silently corrupting the gradients."""
    monkeypatch.setattr(ops, '_SMALL', small)
    C = 4 if (small or DEV == 'cpu') else 32
    graph = CsrGraph.queen_grid(4, 5, normalize=True)
    torch.manual_seed(1)
    model = M.STCGNN(20, C, 2, 2, 1, 16, 1, 2, graph_mode='csr-fixed').to(DEV)
    pair = M._graphs(graph, torch.softmax(torch.randn(C, C), -1).to(DEV), 2, 2)
    X = torch.rand(2, 2, 20, C, 1).to(DEV)
    stacked = model._run_cell_graph(pair, X)
    assert stacked is not None
    loss = stacked.sum()
    with torch.no_grad():
        stacked.mul_(2.0)
    with pytest.raises(RuntimeError, match='modified in place'):
        loss.backward()


@pytest.mark.parametrize('layers,T,horizon,cin', [(2, 3, 2, 1), (3, 2, 2, 4)])
def test_two_launch_cell_backward_option(dev, monkeypatch, layers, T, horizon, cin):
    """The planar cells' backward as two launches (stc_bdg_node_post_bwd_f32 + stc_cell_gates_bwd_planar_f32, with
    the R*H plane stored by the forward) instead of stc_cell_bwd_planar_f32 -- same predictions and gradients."""
    test_cell_graph_equals_the_per_cell_path(dev, monkeypatch, layers, T, horizon, cin, 2, False, one_launch_bwd=False)
