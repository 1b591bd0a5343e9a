"""Self-Masked Representation Training ('Self-Flow') on label + image pairs - the configuration of the reference's `train_self_flow.py`: the
`train_mnist.py` model (class-label token, 28 x 28 image patchified to 14 x 14 x 4 channel-first latents, axial positional embedding, CFG text drop)
inside `SelfMaskedRepTraining`: the student's hidden at `student_layer = -3` goes through a prediction head and is pulled towards the EMA teacher's
final-norm output (`teacher_layer = -1`) by a cosine loss, next to the student's own loss.  One keyword differs from the reference's script:
`use_asymmetric_dropout=False` (the MI355X kernels have no dropout; the teacher's better view is its EMA weights and the deeper layer).
No network here: the "digits" are the ten synthetic stroke templates of examples/label_image_cfg.py.

    python examples/self_flow_label_image.py --steps 300
"""
from __future__ import annotations

import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from transfusion_pytorch_amd import SelfMaskedRepTraining, Transfusion, print_modality_sample          # noqa: E402
from image_flow_unet import Patchify, Unpatchify                                                      # noqa: E402
from label_image_cfg import LabelledStrokes                                                           # noqa: E402


def build_wrapper():
    model = Transfusion(num_text_tokens=10, dim_latent=4, modality_default_shape=(14, 14), modality_encoder=Patchify(), modality_decoder=Unpatchify(),
                        add_pos_emb=True, modality_num_dim=2, prob_uncond=0.1, channel_first_latent=True,
                        transformer=dict(dim=64, depth=4, dim_head=32, heads=8)).cuda()
    return SelfMaskedRepTraining(model, use_asymmetric_dropout=False, student_dropout_rate=0.1, teacher_dropout_rate=0., rep_loss_weight=0.1,
                                 student_layer=-3, teacher_layer=-1).cuda()


def train(ssl_wrapper, optimizer, steps=300, batch_size=16, log=print, quiet=False):
    """the loop of train_self_flow.py:132-146; `optimizer` is torch.optim.Adam(ssl_wrapper.parameters()) or optim.FusedAdam(ssl_wrapper, max_grad_norm=0.5)"""
    loader = ssl_wrapper.student.create_dataloader(LabelledStrokes(), batch_size=batch_size, shuffle=True)
    fused = not isinstance(optimizer, torch.optim.Optimizer)
    history, step = [], 0
    while step < steps:
        for batch in loader:
            step += 1
            ssl_wrapper.train()
            loss, (student_loss, self_flow_loss) = ssl_wrapper(batch)
            loss.backward()
            if not fused:                                                  # (the fused optimizer clips inside its step)
                torch.nn.utils.clip_grad_norm_(list(ssl_wrapper.parameters()), 0.5)
            optimizer.step()
            optimizer.zero_grad()
            ssl_wrapper.update_teacher()
            history.append((loss.item(), student_loss.item(), self_flow_loss.item()))
            if not quiet and step % 50 == 0:
                log(f'{step}: {history[-1][0]:.3f} | ar: {history[-1][1]:.3f} | self flow: {history[-1][2]:.3f}')
            if step >= steps:
                break
    return history


def main(steps=300, batch_size=16, sample=True, fused=False):
    torch.manual_seed(0)
    ssl_wrapper = build_wrapper()
    ema_model = ssl_wrapper.teacher
    if fused:
        from transfusion_pytorch_amd.optim import FusedAdam
        optimizer = FusedAdam(ssl_wrapper, lr=3e-4, max_grad_norm=0.5)
    else:
        optimizer = torch.optim.Adam(ssl_wrapper.parameters(), lr=3e-4)
    history = train(ssl_wrapper, optimizer, steps=steps, batch_size=batch_size)
    out = None
    if sample:
        out = ema_model.sample(max_length=384, cfg_scale=3.0)
        print_modality_sample(out)
    return history, out


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=300)
    ap.add_argument('--batch-size', type=int, default=16)
    ap.add_argument('--no-sample', action='store_true')
    ap.add_argument('--fused', action='store_true', help='optim.FusedAdam(wrapper) instead of torch.optim.Adam(wrapper.parameters())')
    a = ap.parse_args()
    main(a.steps, a.batch_size, not a.no_sample, a.fused)
