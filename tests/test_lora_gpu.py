"""LoRA adapters end to end on the GPU (transfusion_pytorch_amd/lora.py) against the reference fixtures tests/golden/lora_*.pt (tools/make_golden_lora.py:
the unmodified reference with W + s B A as weights; dA = s B^T dW and dB = s dW A^T from its dW in float64).

Gates, those of tests/test_model_gpu.py: loss |delta| <= LOSS_TOL max(1, |ref|), logits rel-Frobenius <= LOGIT_TOL; every adapter tensor's rel-Frobenius error
<= max(GRAD_TOL, 1.5 x the fixture's recorded bf16-autocast deviation of that tensor) - the 1.5 factor is the README's parity rule.  Every test prints its
figures as `LORA <case> ...` lines: profiles/lora_bounds.txt keeps a copy."""
import ctypes
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle.cases import build_case, build_text_case          # noqa: E402

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')
LOSS_TOL, LOGIT_TOL, GRAD_TOL = 1e-3, 1e-2, 4e-2
_FIX = {}


def fixture(name):
    if name not in _FIX:
        _FIX[name] = torch.load(os.path.join(GOLDEN, f'{name}.pt'), weights_only=False)
    return _FIX[name]


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def build_native(cfg, sd):
    from transfusion_pytorch_amd import Transfusion
    dl = cfg.dim_latents if len(cfg.dim_latents) > 1 else cfg.dim_latents[0]
    model = Transfusion(num_text_tokens=cfg.num_text_tokens, dim_latent=dl,
                        transformer=dict(dim=cfg.dim, depth=cfg.depth, dim_head=cfg.dim_head, heads=cfg.heads), prob_uncond=0.)
    model.load_state_dict(sd, strict=True)
    return model.cuda()


def attach(model, g, freeze_base=True):
    """the fixture's adapters on the native model, through the public surface (values by `copy_`, as a user loading a checkpoint would)"""
    from transfusion_pytorch_amd import add_lora_
    add_lora_(model, rank=g['rank'], alpha=g['alpha'], targets=g['targets'], layers=g['layers'], freeze_base=freeze_base)
    prm = dict(model.named_parameters())
    with torch.no_grad():
        for path in g['A']:
            prm[f'lora.{path}.A'].copy_(g['A'][path])
            prm[f'lora.{path}.B'].copy_(g['B'][path])
    return model


def adapted(name, freeze_base=True):
    g = fixture(name)
    if g['kind'] == 'train':
        cfg, sd, batch, times, noise = build_case(g['base_case'])
        inputs = (batch, times, noise)
    else:
        cfg, sd, text = build_text_case(g['base_case'])
        inputs = (text,)
    return g, cfg, attach(build_native(cfg, sd), g, freeze_base).train(), inputs


def step(model, g, inputs):
    if g['kind'] == 'train':
        batch, times, noise = inputs
        if model._noise_override is None:                  # (once: the forward list holds the pointers)
            model._noise_override = {t: v.cuda() for t, v in noise.items()}
        loss = model(batch, times=times)
    else:
        loss = model.forward_text(inputs[0])
    loss.backward()
    torch.cuda.synchronize()
    return loss


def native_logits(model, g, cfg, inputs):
    if g['kind'] == 'train':
        plan = model._live[0]
        return plan.logits.view(plan.b, plan.n, -1)[:, :model._live_n_true, :cfg.vocab].float().cpu()
    with torch.no_grad():
        return model(inputs[0][:, :-1].cuda(), return_loss=False).float().cpu()[:, ::g['row_step']]


def check_adapter_grads(name, model, g):
    worst = (None, 0.)
    for k, ref in g['grads'].items():
        p = dict(model.named_parameters())[f'lora.{k}']
        assert p.grad is not None, k
        assert float(ref.double().norm()) > 0
        e, floor = rel(p.grad, ref), g['bf16_grad_rel'][k]
        tol = max(GRAD_TOL, 1.5 * floor)
        ratio = e / tol
        if ratio > worst[1]:
            worst = (k, ratio)
        print(f'LORA {name} {k} rel {e:.3e} reference bf16 floor {floor:.3e} tol {tol:.3e} ratio {ratio:.3f}')
        assert e <= tol, f'{k}: rel err {e:.3e} over {tol:.3e}'
    print(f'LORA {name} worst adapter gradient ratio {worst[1]:.3f} ({worst[0]})')


@pytest.mark.parametrize('name', ['lora_small2', 'lora_head8', 'lora_text1'])
def test_adapted_step_matches_reference_golden(name):
    g, cfg, model, inputs = adapted(name)
    loss = step(model, g, inputs)
    ref = float(g['loss'])
    print(f'LORA {name} loss native {float(loss):.6f} reference {ref:.6f} (without adapters {float(g["plain_loss"]):.6f})')
    assert abs(float(loss) - ref) <= LOSS_TOL * max(1., abs(ref))
    e = rel(native_logits(model, g, cfg, inputs), g['logits'])
    print(f'LORA {name} logits rel {e:.3e} (reference bf16 floor {g["bf16_logits_rel"]:.3e})')
    assert e <= LOGIT_TOL
    # everything else is frozen: no gradient on any native parameter, all-zero bits in the flat gradient buffer
    assert all(p.grad is None for p in model.store.params.values())
    assert not bool(model.store.grad.view(torch.int32).any())
    check_adapter_grads(name, model, g)


def test_trainable_base_weight_beside_its_adapter_matches_reference_dw():
    g, cfg, model, inputs = adapted('lora_small2')
    w = model.store.params[g['dW_name']]
    w.requires_grad_(True)
    step(model, g, inputs)
    e = rel(w.grad, g['dW'])
    print(f'LORA lora_small2 base weight {g["dW_name"]} beside its adapter rel {e:.3e}')
    assert e <= GRAD_TOL
    assert all(p.grad is None for n, p in model.store.params.items() if n != g['dW_name'])
    check_adapter_grads('lora_small2+base', model, g)


def test_gradients_accumulate_over_micro_batches_and_restart_from_none():
    g, cfg, model, inputs = adapted('lora_head8')
    step(model, g, inputs)
    from transfusion_pytorch_amd import lora_parameters
    once = [p.grad.clone() for p in lora_parameters(model)]
    step(model, g, inputs)
    for p, o in zip(lora_parameters(model), once):
        assert rel(p.grad, 2 * o) <= 1e-6
    model.zero_grad(set_to_none=True)
    step(model, g, inputs)
    for p, o in zip(lora_parameters(model), once):
        # (the adapter kernels repeat their bits - tests/test_lora_kernels_gpu.py; the dY they read comes down a chain this test does not pin to the bit)
        assert rel(p.grad, o) <= 1e-6, 'a fresh accumulation starts from zero'


def test_merge_keeps_logits_bits_and_greedy_tokens():
    from transfusion_pytorch_amd import merge_lora_
    g, cfg, model, inputs = adapted('lora_text1')
    text = inputs[0]
    model.eval()
    prompt = text[:, :16].clone().cuda()
    prompt[prompt < 0] = 0
    with torch.no_grad():
        before = model(text[:, :-1].cuda(), return_loss=False).clone()
        gen_before = model.generate_text_only(prompt, 16 + 12, temperature=0.).clone()
    keys = [k for k in model.state_dict() if k.startswith('lora.')]
    assert keys
    base_before = model.store.flat.clone()
    merge_lora_(model)
    assert not [k for k in model.state_dict() if k.startswith('lora.')] and model.store.lora is None
    assert not torch.equal(base_before, model.store.flat), 'the masters now hold W_eff'
    with torch.no_grad():
        after = model(text[:, :-1].cuda(), return_loss=False)
        gen_after = model.generate_text_only(prompt, 16 + 12, temperature=0.)
    assert before.dtype == after.dtype and torch.equal(before, after) and bool(torch.isfinite(before).all()), 'logits before and after merge_lora_ are bit-identical'
    assert torch.equal(gen_before, gen_after)
    e = rel(after.float().cpu()[:, ::g['row_step']], g['logits'])
    assert e <= LOGIT_TOL


def test_two_fused_adam_steps_move_only_the_adapters():
    from transfusion_pytorch_amd import lora_parameters
    from transfusion_pytorch_amd.optim import FusedAdam
    g, cfg, model, inputs = adapted('lora_head8')
    opt = FusedAdam(model, lr=1e-3, max_grad_norm=1.0)
    flat0 = model.store.flat.clone()
    vals0 = [p.detach().clone() for p in lora_parameters(model)]
    losses = []
    for _ in range(2):
        opt.zero_grad()
        losses.append(float(step(model, g, inputs)))
        opt.step()
    torch.cuda.synchronize()
    assert torch.equal(flat0.view(torch.int32), model.store.flat.view(torch.int32)), 'the frozen flat buffer keeps its bits'
    assert all(not torch.equal(a, p.detach()) for a, p in zip(vals0, lora_parameters(model))), 'every adapter tensor moved'
    third = float(step(model, g, inputs))
    print(f'LORA lora_head8 FusedAdam losses {losses[0]:.6f} {losses[1]:.6f} {third:.6f}')
    assert losses[1] != losses[0] and third != losses[1], 'the shadows follow the adapters: each step sees the new W_eff'
    assert third < losses[0]


def _fingerprint(L):
    from transfusion_pytorch_amd import capi
    arr = L.native()
    out = ctypes.c_int64(0)
    capi.check(capi.lib().tfx_list_fingerprint(ctypes.byref(arr), len(L), ctypes.byref(out)), 'tfx_list_fingerprint')
    return len(L), out.value


def _same_forward(model, loss, logits0, loss0):
    """the forward's bits: every logit (GEMM outputs, no atomics) equals bit for bit.  The scalar loss is summed from them with fp32 atomics over the blocks of
    tfx_ce_fwd_bwd / tfx_mse_fwd_bwd, so its last bit follows the blocks' order from run to run on an unchanged model too: it is held to 2 ulp."""
    plan = model._live[0]
    assert torch.equal(plan.logits.view(torch.int32), logits0.view(torch.int32))
    assert abs(float(loss) - float(loss0)) <= 2 * 2.0 ** -23 * abs(float(loss0))


def test_model_that_gained_and_lost_adapters_runs_the_parents_lists():
    from transfusion_pytorch_amd import add_lora_, remove_lora_
    cfg, sd, batch, times, noise = build_case('small2')
    model = build_native(cfg, sd).train()
    g = dict(kind='train')
    keys0 = list(model.state_dict())
    loss0 = step(model, g, (batch, times, noise)).detach().clone()
    plan = model._live[0]
    fp0 = (_fingerprint(plan.fwd), _fingerprint(plan.bwd))
    logits0 = plan.logits.clone()
    grads0 = model.store.grad.clone()
    # adapters with B = 0 beside a trainable base: the same forward, a longer backward list
    add_lora_(model, rank=8, layers=(1, 3), freeze_base=False)
    model.zero_grad(set_to_none=True)
    loss1 = step(model, g, (batch, times, noise)).detach().clone()
    assert model._live[0] is plan
    _same_forward(model, loss1, logits0, loss0)                  # B = 0: W_eff holds the bits of W
    assert _fingerprint(plan.fwd) == fp0[0] and _fingerprint(plan.bwd)[0] > fp0[1][0]
    assert rel(model.store.grad, grads0) <= 1e-5, 'the base gradients do not see the adapter launches (fp32 atomics: equal up to summation order)'
    remove_lora_(model)
    model.zero_grad(set_to_none=True)
    loss2 = step(model, g, (batch, times, noise)).detach().clone()
    assert list(model.state_dict()) == keys0
    _same_forward(model, loss2, logits0, loss0)
    assert (_fingerprint(plan.fwd), _fingerprint(plan.bwd)) == fp0, 'the lists of a model without adapters are the lists it always built'
    assert rel(model.store.grad, grads0) <= 1e-5


def test_unsupported_combinations_raise_while_adapters_are_attached():
    from transfusion_pytorch_amd import EMA, SelfMaskedRepTraining, lora_parameters, remove_lora_
    from transfusion_pytorch_amd.optim import FusedMuon
    g, cfg, model, inputs = adapted('lora_head8')
    for make in (model.create_ema, lambda: EMA(model), lambda: SelfMaskedRepTraining(model, use_asymmetric_dropout=False)):
        with pytest.raises(NotImplementedError, match='merge_lora_'):
            make()
    with pytest.raises(NotImplementedError, match='Muon'):
        FusedMuon(model, muon_params=model.muon_parameters() + lora_parameters(model)[:1])
    remove_lora_(model)
    model.create_ema()
