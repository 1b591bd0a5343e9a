"""Write tests/golden/muon_names.json: the names of the UNMODIFIED reference's `Transfusion.muon_parameters()` (transfusion.py:1657-1672), in
its order, for three configurations of oracle/cases.py (only where the reference is present).

    python tools/make_golden_muon.py

TEST INFRASTRUCTURE ONLY.  The fixture is a list of parameter names per case; tests/test_muon_cpu.py compares the native model's list with it.
"""
from __future__ import annotations

import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle.cases import CASES, default_shapes                                            # noqa: E402
from oracle.ref_runner import import_reference                                            # noqa: E402
from oracle.transfusion_oracle import OracleConfig                                        # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'muon_names.json')
NAMES = ('small2', 'head8', 'canon512')


def make(name):
    tp = import_reference()
    cfg = OracleConfig(**CASES[name][0])
    dl = cfg.dim_latents if len(cfg.dim_latents) > 1 else cfg.dim_latents[0]
    torch.manual_seed(0)
    m = tp.Transfusion(num_text_tokens=cfg.num_text_tokens, dim_latent=dl, modality_default_shape=default_shapes(cfg),
                       transformer=dict(dim=cfg.dim, depth=cfg.depth, dim_head=cfg.dim_head, heads=cfg.heads),
                       modality_processing='flat', prob_uncond=0.)
    by_id = {id(p): n for n, p in m.named_parameters()}
    return [by_id[id(p)] for p in m.muon_parameters()]


def make_all():
    return {name: make(name) for name in NAMES}


if __name__ == '__main__':
    with open(OUT, 'w') as f:
        json.dump(make_all(), f, indent=1)
        f.write('\n')
    print('wrote', OUT)
