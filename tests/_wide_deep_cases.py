"""Model cases outside / at the edge of the pull-form region (not collected: no test_ prefix; imports no GPU code).

`engine.pull_form_ok` (depth <= PULL_MAX_DEPTH and dim <= PULL_MAX_DIM) decides whether a training plan runs the AttentionResidual backward in pull
form; `Plan._side_stream` (depth <= 30 and dim <= 1024) whether its weight-gradient GEMMs go to the side stream.  Every other model test sits at
dim <= 1024 and depth <= 24.  These are the smallest shapes that cross each boundary (dim is a multiple of 64: 1088 is the first above 1024), built
exactly as tests/test_model_gpu.py::test_odd_configurations_match_live_oracle builds its configurations.

Shared by tests/test_wide_deep_cpu.py (the oracle runs, every gradient is above the comparison's floor, the expected plan form) and
tests/test_push_form_gpu.py (the native step against the live oracle)."""
import functools
from types import SimpleNamespace

NORM_FLOOR = 1e-7            # the GPU comparison skips a parameter whose oracle gradient norm is below this (tests/test_model_gpu.py)

# name: dim, depth, heads, dim_latents, dim_head | expected: pull form, side stream, U-Net skip pairs {late layer: early layer whose input it pops}
_pairs = lambda depth: {i: depth - 1 - i for i in range(depth) if i >= depth / 2}          # (last in, first out; an odd depth's middle layer has no skip)
CASES = {
    'w1088x2': SimpleNamespace(dim=1088, depth=2,  heads=2, dls=(16,),    dim_head=64, pull=False, side=False, skips={1: 0}),
    'w1088x3': SimpleNamespace(dim=1088, depth=3,  heads=1, dls=(16, 24), dim_head=64, pull=False, side=False, skips={2: 0}),
    'd30':     SimpleNamespace(dim=64,   depth=30, heads=2, dls=(16,),    dim_head=64, pull=True,  side=True,  skips=_pairs(30)),
    'd32':     SimpleNamespace(dim=64,   depth=32, heads=2, dls=(16,),    dim_head=64, pull=True,  side=False, skips=_pairs(32)),
    'd33':     SimpleNamespace(dim=64,   depth=33, heads=2, dls=(16,),    dim_head=64, pull=False, side=False, skips=_pairs(33)),
    'd34':     SimpleNamespace(dim=64,   depth=34, heads=2, dls=(16, 24), dim_head=64, pull=False, side=False, skips=_pairs(34)),
    'd33h32':  SimpleNamespace(dim=128,  depth=33, heads=4, dls=(16,),    dim_head=32, pull=False, side=False, skips=_pairs(33)),
}
N_SKIP = dict(w1088x2=1, w1088x3=1, d30=15, d32=16, d33=16, d34=17, d33h32=16)          # (the table of the cases, counted by hand: _pairs must agree)


def config(name):
    from oracle.transfusion_oracle import OracleConfig
    c = CASES[name]
    return OracleConfig(num_text_tokens=96, dim=c.dim, depth=c.depth, dim_latents=c.dls, heads=c.heads, dim_head=c.dim_head)


def dims(name):
    """the native model's dimensions of the case (what engine.pull_form_ok, Plan._side_stream and engine.skip_sources read)"""
    from transfusion_pytorch_amd.params import ModelDims
    c = CASES[name]
    return ModelDims(num_text_tokens=96, dim=c.dim, depth=c.depth, heads=c.heads, dim_head=c.dim_head, dim_latents=c.dls)


@functools.lru_cache(maxsize=None)
def build(name):
    """(cfg, state dict, batch, times, noise) - pure functions of the case's tag; built once per process, never modified by a test"""
    from oracle import detdata as D
    c = CASES[name]
    cfg = config(name)
    tag = f'wide/{c.dim}/{c.depth}'
    batch = D.ragged_batch(f'{tag}/b', 3, cfg.num_text_tokens, cfg.dim_latents)
    times = D.det_times(f'{tag}/t', batch); noise = D.det_noise(f'{tag}/n', batch, cfg.num_modalities)
    sd = D.det_state_dict(cfg.state_dict_shapes(), tag=tag)
    return cfg, sd, batch, times, noise


@functools.lru_cache(maxsize=None)
def oracle_step(name):
    """one training step of the CPU oracle (fp32) on the case: loss, logits and every trainable parameter's gradient; run once per process"""
    from oracle.cases import with_grad
    from oracle.transfusion_oracle import forward_train
    cfg, sd, batch, times, noise = build(name)
    sdg = with_grad(sd)
    ref = forward_train(sdg, cfg, batch, times, noise, return_all=True)
    ref['loss'].backward()
    grads = {k: p.grad.detach() for k, p in sdg.items() if p.requires_grad and p.grad is not None}
    trainable = [k for k, p in sdg.items() if p.requires_grad]
    return SimpleNamespace(loss=float(ref['loss'].detach()), logits=ref['logits'].detach(), grads=grads, trainable=trainable)
