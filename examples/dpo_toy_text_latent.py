"""Direct preference optimisation on the native MI355X path, on synthetic pairs: the per-token losses of the fused step
(`model.set_token_losses_()`: every training call also returns a `TokenLosses`) are all a DPO loss needs.

  policy      LoRA adapters on a frozen base (`add_lora_`): only the adapters train
  reference   a deep copy of the base taken BEFORE the adapters were added, run under `torch.no_grad()` - its weights never move
  one batch   chosen and rejected samples go through ONE policy forward (the engine keeps the activations of a model's latest forward only): rows
              0 .. p - 1 are the chosen samples, rows p .. 2 p - 1 the rejected ones
  loss        -logsigmoid(beta ((logp_policy(chosen) - logp_policy(rejected)) - (logp_ref(chosen) - logp_ref(rejected)))), logp(sample) = -TokenLosses.text.sum(1)

Every sample is a short text followed by a small latent (the toy layout of examples/toy_text_latent.py, text first: under the causal mask the text's
log-probability does not see the latent's noise).  A chosen text counts upwards from a random start, a rejected one is random tokens.

    python examples/dpo_toy_text_latent.py --steps 40
"""
from __future__ import annotations

import argparse
import copy
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from transfusion_pytorch_amd import Transfusion, add_lora_, lora_parameters          # noqa: E402

VOCAB, LENGTH = 32, 12


def make_pairs(pairs=4, seed=0):
    """(chosen samples, rejected samples): each sample = [text (LENGTH,), latent (2, 16)]"""
    g = torch.Generator().manual_seed(seed)
    latent = lambda: torch.randn(2, 16, generator=g)
    chosen = [[(int(torch.randint(0, VOCAB, (1,), generator=g)) + torch.arange(LENGTH)) % VOCAB, latent()] for _ in range(pairs)]
    rejected = [[torch.randint(0, VOCAB, (LENGTH,), generator=g), latent()] for _ in range(pairs)]
    return chosen, rejected


def sequence_logprob(model, batch):
    """log-probability of every sample's text under `model`: minus the sum of its per-token losses (differentiable when gradients are enabled)"""
    _, tok = model(batch)                                    # (loss, TokenLosses): the switch is on, see main
    return -tok.text.sum(dim=1)


def main(steps=40, pairs=4, beta=0.5, lr=5e-3, rank=8, log=print):
    torch.manual_seed(0)
    model = Transfusion(num_text_tokens=VOCAB, dim_latent=16, modality_default_shape=(2,), prob_uncond=0.,
                        transformer=dict(dim=64, depth=2, dim_head=32, heads=2)).cuda()
    reference = copy.deepcopy(model).eval().set_token_losses_()      # before the adapters: the frozen reference model (a copy starts with the switch off)
    before = {k: v.detach().clone() for k, v in reference.state_dict().items()}
    model.set_token_losses_()
    add_lora_(model, rank=rank)                              # freezes the base, adapters start at zero: policy == reference at step 0
    opt = torch.optim.Adam(lora_parameters(model), lr=lr)
    chosen, rejected = make_pairs(pairs)
    batch, p = chosen + rejected, pairs
    losses = []
    for step in range(1, steps + 1):
        with torch.no_grad():
            ref = sequence_logprob(reference, batch)
        pol = sequence_logprob(model, batch)                 # one policy forward over chosen + rejected
        margin = (pol[:p] - pol[p:]) - (ref[:p] - ref[p:])
        loss = -torch.nn.functional.logsigmoid(beta * margin).mean()
        loss.backward()                                      # the row gradients enter the hand-written backward as per-row factors
        opt.step()
        opt.zero_grad()
        losses.append(float(loss.detach()))
        if step % 10 == 0 or step == 1:
            log(f'{step}: dpo loss {losses[-1]:.4f}  mean margin {float(margin.detach().mean()):+.3f}')
    moved = [k for k, v in reference.state_dict().items() if not torch.equal(v, before[k])]
    return losses, moved


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=40)
    ap.add_argument('--pairs', type=int, default=4)
    ap.add_argument('--beta', type=float, default=0.5)
    a = ap.parse_args()
    losses, moved = main(steps=a.steps, pairs=a.pairs, beta=a.beta)
    print(f'first {losses[0]:.4f} last {losses[-1]:.4f}; reference parameters that moved: {len(moved)}')
