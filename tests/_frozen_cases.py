"""Freeze sets of the frozen-parameter tests (tests/test_frozen_cpu.py, tests/test_frozen_gpu.py): predicates over the names of the NATIVE parameters
(`model.store.params`, the reference's `named_parameters()` names).  A predicate answers "does this parameter TRAIN in the set"; everything else
of the native model is frozen with `requires_grad_(False)`.  Parameters outside the flat buffer (positional-embedding MLPs, the user's encoders /
decoders) are not touched: they follow `requires_grad` through autograd as they always did."""
import torch

HEADS = ('model_to_latent_projs.', 'to_text_logits.weight')


def _layer(name):
    return int(name.split('.')[2]) if name.startswith('transformer.layers.') else None


SETS = {
    'heads':       lambda n, depth: n.startswith(HEADS),
    'modality1':   lambda n, depth: n.startswith(('latent_to_model_projs.1.', 'model_to_latent_projs.1.')),
    'top_half':    lambda n, depth: n.startswith(HEADS) or n == 'transformer.norm.gamma' or (_layer(n) is not None and _layer(n) >= depth / 2),
    'bias_gain':   lambda n, depth: n.endswith(('bias', 'gamma', 'layerscale', 'pseudo_queries')),
    'v_only':      lambda n, depth: '.to_v.' in n,
    'text_frozen': lambda n, depth: n not in ('text_embed.weight', 'to_text_logits.weight'),
    'all_frozen':  lambda n, depth: False,
}


def trainable_names(names, depth, set_name):
    return [n for n in names if SETS[set_name](n, depth)]


def freeze(model, set_name):
    """apply the set to the native parameters of `model`; returns (frozen names, trainable names)"""
    ps = model.store
    keep = set(trainable_names(ps.params, ps.md.depth, set_name))
    for n, p in ps.params.items():
        p.requires_grad_(n in keep)
    return [n for n in ps.params if n not in keep], [n for n in ps.params if n in keep]


def unfreeze(model):
    for p in model.store.params.values():
        p.requires_grad_(True)


def brute_force_ranges(store, frozen):
    """[start, end) ranges of the frozen segments by walking `store.offsets` element by element: a boolean mask over the flat buffer (a segment's
    padding to a multiple of 4 belongs to it), then its runs"""
    mask = torch.zeros(store.numel + 1, dtype=torch.bool)
    for n in frozen:
        off, shape = store.offsets[n]
        size = int(torch.Size(shape).numel())
        mask[off:off + -(-size // 4) * 4] = True
    edges = (mask[1:] != mask[:-1]).nonzero().flatten().tolist()
    starts = ([0] if mask[0] else []) + [e + 1 for e in edges]
    return [(a, b) for a, b in zip(starts[0::2], starts[1::2])]
