"""LoRA adapters without a GPU: the fixtures exercise the adapters, the public surface of transfusion_pytorch_amd/lora.py, the C ABI of csrc/lora.hip,
and the float64 restatements of the two adapter-gradient kernels (tests/_lora_cases.py) against torch autograd."""
import ctypes
import os
import sys

import pytest
import torch

from transfusion_pytorch_amd import Transfusion, add_lora_, capi, lora_parameters, merge_lora_, remove_lora_
from transfusion_pytorch_amd.lora import TARGETS
from transfusion_pytorch_amd.optim import FusedAdam, FusedMuon

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _lora_cases as C  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')
LOSS_TOL = 1e-3
FIXTURES = ('lora_small2', 'lora_head8', 'lora_text1')


def native(depth=4, dim_head=8, heads=4, dim=64):
    return Transfusion(num_text_tokens=32, dim_latent=8, transformer=dict(dim=dim, depth=depth, dim_head=dim_head, heads=heads))


# ---------------------------------------------------------------------------------------------- fixtures
@pytest.mark.parametrize('name', FIXTURES)
def test_fixture_cannot_be_passed_by_a_model_that_ignores_the_adapters(name):
    g = torch.load(os.path.join(GOLDEN, f'{name}.pt'), weights_only=False)
    assert abs(float(g['loss']) - float(g['plain_loss'])) >= 10 * LOSS_TOL
    assert set(g['grads']) == {f'{p}.{k}' for p in g['A'] for k in 'AB'} == set(g['bf16_grad_rel'])
    for k, v in g['grads'].items():
        assert float(v.double().norm()) > 0 and bool(torch.isfinite(v).all()), k
    for p in g['A']:
        assert float(g['A'][p].abs().max()) > 0 and float(g['B'][p].abs().max()) > 0
        assert g['A'][p].shape[0] == g['B'][p].shape[1] == g['rank']
    assert g['scale'] == g['alpha'] / g['rank']
    assert os.path.getsize(os.path.join(GOLDEN, f'{name}.pt')) < 1 << 20


def test_fixture_cases_are_the_ones_the_tool_names():
    g = {n: torch.load(os.path.join(GOLDEN, f'{n}.pt'), weights_only=False) for n in FIXTURES}
    assert (g['lora_small2']['base_case'], g['lora_small2']['rank'], g['lora_small2']['layers'], g['lora_small2']['targets']) == ('small2', 8, (1, 3), TARGETS)
    assert (g['lora_head8']['base_case'], g['lora_head8']['rank'], g['lora_head8']['targets']) == ('head8', 4, ('to_qk', 'to_v', 'to_out'))
    assert (g['lora_text1']['base_case'], g['lora_text1']['rank'], g['lora_text1']['kind']) == ('text1', 16, 'text')


# ---------------------------------------------------------------------------------------------- surface
def test_state_dict_keys_parameter_order_and_shapes():
    m = native()
    keys0, n0 = list(m.state_dict()), len(list(m.parameters()))
    add_lora_(m, rank=4, layers=(3, 1))
    new = [k for k in m.state_dict() if k not in keys0]
    want = [f'lora.transformer.layers.{i}.{mod}.{k}' for i in (1, 3)
            for mod in ('1.fn.to_qk.0', '1.fn.to_v.0', '1.fn.to_out.1', '2.fn.net.0', '2.fn.net.3') for k in 'AB']
    assert new == want and list(m.state_dict())[:len(keys0)] == keys0
    names = [n for n, _ in m.named_parameters()]
    assert names[-len(want):] == want and len(names) == n0 + len(want)
    by_name = dict(m.named_parameters())
    assert [id(p) for p in lora_parameters(m)] == [id(by_name[k]) for k in want]
    md = m.md
    shapes = {'to_qk': (2 * md.hd, md.dim), 'to_v': (md.hd, md.dim), 'to_out': (md.dim, md.hd), 'net.0': (2 * md.di, md.dim), 'net.3': (md.dim, md.di)}
    for a in m.store.lora.adapters.values():
        d_out, d_in = shapes[a.target]
        assert tuple(a.A.shape) == (4, d_in) and tuple(a.B.shape) == (d_out, 4) and a.A.dtype == a.B.dtype == torch.float32
        assert tuple(m.store.params[a.weight].shape) == (d_out, d_in)
        assert not bool(a.B.detach().any()) and 0 < float(a.A.detach().abs().max()) <= d_in ** -0.5 + 1e-6      # nn.Linear's U(-1/sqrt(fan_in), ..)
        assert a.s == 1.0
    # a second call adds to the set, in (layer, target) order whatever the order of the calls
    add_lora_(m, rank=2, alpha=8, targets=('to_out',), layers=(0,))
    assert [n for n, _ in m.named_parameters()][n0:n0 + 2] == ['lora.transformer.layers.0.1.fn.to_out.1.A', 'lora.transformer.layers.0.1.fn.to_out.1.B']
    assert m.store.lora.get(0, 'to_out').s == 4.0
    # load_state_dict loads the adapters
    sd = {k: torch.full_like(v, 0.25) if k.startswith('lora.') else v for k, v in m.state_dict().items()}
    m.load_state_dict(sd, strict=True)
    assert all(bool((p == 0.25).all()) for p in lora_parameters(m))


def test_value_errors_and_refusals():
    m = native()
    for bad in (0, 65, -1, 2.5, True):
        with pytest.raises(ValueError):
            add_lora_(m, rank=bad)
    with pytest.raises(ValueError):
        add_lora_(m, targets=('to_qk', 'nonsense'))
    for i in (4, -1):
        with pytest.raises(ValueError):
            add_lora_(m, layers=(i,))
    for t in ('to_gates', 'to_text_logits', 'text_embed', 'to_film', 'to_ada_ln_zero', 'skip'):
        with pytest.raises(NotImplementedError):
            add_lora_(m, targets=(t,))
    assert m.store.lora is None and not [k for k in m.state_dict() if k.startswith('lora.')], 'a refused call attaches nothing'
    add_lora_(m, rank=64, targets=('to_v',), layers=(2,))
    with pytest.raises(ValueError, match='already has an adapter'):
        add_lora_(m, rank=1, targets=('to_out', 'to_v'), layers=(2,))
    assert len(lora_parameters(m)) == 2
    with pytest.raises(NotImplementedError, match='merge_lora_'):
        m.create_ema()
    with pytest.raises(NotImplementedError, match='Muon'):
        FusedMuon(m, muon_params=[lora_parameters(m)[0]])
    with pytest.raises(capi.TfxError):
        merge_lora_(m)                                     # the merge is a HIP kernel: no CPU fallback


def test_external_parameters_frozen_set_and_remove():
    m = native()
    keys0, ext0, frozen0 = list(m.state_dict()), m.external_parameters(), m.store.frozen_names()
    assert ext0 == [] and frozen0 == frozenset()
    assert lora_parameters(m) == [] and remove_lora_(m) is m
    add_lora_(m, rank=8, targets=('to_qk', 'net.3'))
    assert m.store.frozen_names() == frozenset(m.store.params), 'freeze_base: every native parameter'
    assert [id(p) for p in m.external_parameters()] == [id(p) for p in lora_parameters(m)] and len(lora_parameters(m)) == 2 * 2 * 4
    lora_parameters(m)[0].requires_grad_(False)
    assert [id(p) for p in m.external_parameters()] == [id(p) for p in lora_parameters(m)[1:]]
    key = m.store.lora.key()
    assert len(key) == 8 and key[0][2:] == (False, True)
    opt = FusedAdam(m, lr=1e-3)
    assert {id(p) for p in opt.ext_params} == {id(p) for p in lora_parameters(m)[1:]}
    v0 = m.store.params_version()
    with torch.no_grad():
        lora_parameters(m)[3].add_(1.)
    assert m.store.params_version() != v0, 'a write to an adapter moves params_version(): the shadows are rebuilt'
    remove_lora_(m)
    assert list(m.state_dict()) == keys0 and m.external_parameters() == [] and m.store.lora is None
    assert m.store.frozen_names() == frozenset(m.store.params), 'removing the adapters does not thaw the base'
    m2 = native()
    add_lora_(m2, rank=8, freeze_base=False)
    assert m2.store.frozen_names() == frozenset()


# ---------------------------------------------------------------------------------------------- ABI
def test_abi_entry_points_op_numbers_and_version():
    for fn in ('tfx_lora_merge', 'tfx_lora_down', 'tfx_lora_grad', 'tfx_lora_grad_plan'):
        assert fn in capi.FUNCTIONS and hasattr(capi.lib(), fn)
    ops = {k: v for k, v in capi.ENUMS.items() if k.startswith('TFX_OP_LORA')}
    assert set(ops) == {'TFX_OP_LORA_MERGE', 'TFX_OP_LORA_DOWN', 'TFX_OP_LORA_GRAD'} and set(ops.values()) <= {28, 29, 30, 31}
    assert len(set(ops.values())) == 3 and capi.ENUMS['TFX_OP_OUTPUT_TO_FLOW'] == 32
    others = [v for k, v in capi.ENUMS.items() if k.startswith('TFX_OP_') and k not in ops]
    assert not set(others) & set(ops.values())
    v = capi.lib().tfx_version()
    assert b'lora' in v and v.endswith(b'-frozen') and v.index(b'ablate') < v.index(b'lora') < v.index(b'frozen')
    for s in ('tfx_lora_merge_args', 'tfx_lora_down_args', 'tfx_lora_grad_args'):
        assert s in capi.STRUCTS


def test_grad_plan_is_host_logic_with_fixed_row_runs():
    def plan(M, K, r):
        a = capi.make_args('tfx_lora_grad_args', M=M, K=K, r=r, r_pad=C.r_pad_of(r), ldp=C.r_pad_of(r), ldq=K)
        ch, grid, fl = ctypes.c_int32(-1), ctypes.c_int32(-1), ctypes.c_int64(-1)
        assert capi.lib().tfx_lora_grad_plan(ctypes.byref(a), ctypes.byref(ch), ctypes.byref(grid), ctypes.byref(fl)) == 0
        return ch.value, grid.value, fl.value
    assert plan(64, 64, 8) == (1, 1, 32 * 128) and plan(129, 64, 8)[0] == 3 and plan(128, 64, 8)[0] == 2
    assert plan(65536, 512, 16) == (128, 512, 128 * 32 * 512)
    assert plan(1000, 520, 64) == (16, 16 * 5, 16 * 64 * 640)


# ---------------------------------------------------------------------------------------------- the restatements against autograd
@pytest.mark.parametrize('M,K,N,r,s', [(70, 64, 200, 8, 2.0), (192, 200, 64, 24, 0.5), (129, 520, 136, 1, 1.0)])
def test_float64_restatements_match_autograd(M, K, N, r, s):
    g = torch.Generator().manual_seed(M + K + N + r)
    X = torch.randn(M, K, generator=g, dtype=torch.float64)
    dY = torch.randn(M, N, generator=g, dtype=torch.float64)
    W = torch.randn(N, K, generator=g, dtype=torch.float64)
    A = torch.randn(r, K, generator=g, dtype=torch.float64, requires_grad=True)
    B = torch.randn(N, r, generator=g, dtype=torch.float64, requires_grad=True)
    Weff = W + s * (B @ A)
    assert torch.equal(Weff.detach(), C.merge64(W, B.detach(), A.detach(), s))
    ((X @ Weff.T) * dY).sum().backward()
    rp = C.r_pad_of(r)
    R_a = torch.zeros(rp, K, dtype=torch.float64); R_a[:r] = A.detach()
    R_b = torch.zeros(rp, N, dtype=torch.float64); R_b[:r] = B.detach().T
    U, dU = C.down64(X, R_a), C.down64(dY, R_b)
    assert U.shape == dU.shape == (M, rp) and not bool(U[:, r:].any())
    dBT = C.grad64(U, dY, s, r)
    dA = C.grad64(dU, X, s, r)
    assert torch.allclose(dA, A.grad, rtol=1e-10, atol=1e-10) and torch.allclose(dBT.T, B.grad, rtol=1e-10, atol=1e-10)


def test_case_builders_are_consistent():
    for r in C.RANKS:
        c = C.build_grad(70, 200, r, alpha=0.75, accumulate=1)
        assert c.ref.shape == c.pick(c.buf).shape == (r, 200) and bool((c.tol > 0).all())
        m = C.build_grad(70, 200, r, alpha=0.75, accumulate=0, mapped=True)
        assert m.ref.shape == m.pick(m.buf).shape and int(m.written.sum()) == m.ref.numel()
        d = C.build_down(70, 200, r)
        assert d.ref.shape == (70, C.r_pad_of(r)) and not bool(d.ref[:, r:].any())
