"""Self-Masked Representation Training ('Self-Flow'; reference SelfMaskedRepTraining, T:3452-3569) on hidden taps of the fused step.

    student_loss, student_hiddens, times = student(batch, return_loss=True, return_hiddens=True, return_times=True)
    teacher_hiddens                      = teacher.ema_model(batch, times=times, ...)            (no gradient, its own noise)
    pred  = student_predict_head(student_hiddens[student_layer])                                  RMSNorm(dim) -> FeedForward(dim)
    rep   = loss_fn(pred, teacher_hiddens[teacher_layer])                                         default: 1 - cosine similarity, mean over b * n
    total = student_loss + rep * rep_loss_weight

The student's hidden leaves the fused step as a view of the plan's own buffer and the gradient of the head's input goes back in as a hidden tap
(engine.Plan.set_taps).  The head runs on the library's kernels over the plan's (b, n_pad) token rows - tfx_rmsnorm_fwd / bwd, tfx_gemm_nt with the
GEGLU epilogues, tfx_gemm_tn for the weight and bias gradients - and the default loss is one launch, tfx_cosine_fwd_bwd.  Any other `loss_fn` gets
`pred` and the teacher's hidden as (b, n, dim) PyTorch tensors; its gradient comes back into the head's native backward.

What is built is the reference's `use_asymmetric_dropout=False` mode: the kernels have no dropout (Transformer(dropout=...) raises), so the
default `use_asymmetric_dropout=True` raises at construction instead of training something else without saying so.
"""
from __future__ import annotations

import ctypes
from itertools import chain

import torch
import torch.nn.functional as F
from torch import nn

from . import capi, engine
from .params import geglu_phys_to_ref_rows, pad_to

BF16 = torch.bfloat16


def default_rep_loss_fn(pred, target):                    # T:3456-3458
    cos_sim = F.cosine_similarity(pred, target, dim=-1)
    return 1. - cos_sim.mean()


class _HeadNorm(nn.Module):
    """parameter holder of the head's RMSNorm (T:779-786): y = x / |x| * sqrt(dim) * (gamma + 1)"""

    def __init__(self, dim):
        super().__init__()
        self.gamma = nn.Parameter(torch.zeros(dim))


class _HeadFeedForward(nn.Module):
    """parameter holder of the head's FeedForward (T:836-857): net = [Linear(dim, 2 di), GEGLU, Dropout, Linear(di, dim)], di = int(dim * 8 / 3)"""

    def __init__(self, dim):
        super().__init__()
        di = int(dim * 4 * 2 / 3)
        self.net = nn.Sequential(nn.Linear(dim, di * 2), nn.Identity(), nn.Identity(), nn.Linear(di, dim))


def _head_params(head):
    return (head[0].gamma, head[1].net[0].weight, head[1].net[0].bias, head[1].net[3].weight, head[1].net[3].bias)


class _Head:
    """native forward / backward of student_predict_head over T token rows: bf16 shadows of the five fp32 parameters in kernel layout (rebuilt
    when a parameter changed: version counters and addresses), work buffers per row count"""

    def __init__(self, owner, dim):
        self.owner = owner
        self.d, self.di = dim, int(dim * 4 * 2 / 3)
        self.dip = pad_to(self.di, 64)
        self.shadows, self._ver, self.bufs = None, None, {}

    def params(self):
        return _head_params(self.owner.student_predict_head)

    def _refresh(self, stream):
        ps = self.params()
        for p in ps:
            if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
                raise capi.TfxError('student_predict_head: the parameters must be contiguous fp32 tensors on the GPU (wrapper.cuda())')
        ver = tuple((p.data_ptr(), p._version) for p in ps) + (self.owner._head_epoch,)
        if ver == self._ver:
            return
        d, di, dip = self.d, self.di, self.dip
        dev = ps[0].device
        if self.shadows is None or self.shadows['ff1'].device != dev:
            z = lambda *s, dtype=BF16: torch.zeros(*s, device=dev, dtype=dtype)
            self.shadows = dict(ff1=z(2 * dip, d), ff1_t=z(d, 2 * dip), ff2=z(d, dip), ff2_t=z(dip, d), ff1b=z(2 * dip, dtype=torch.float32),
                                gmap=torch.from_numpy(geglu_phys_to_ref_rows(di, dip)).to(dev))
        S = self.shadows
        _, w1, b1, w2, _ = ps

        def cast(src, ld_src, Rs, Cs, dst, rowmap=None, transpose=False, n_rows_logical=None):
            a = capi.make_args('tfx_cast_args', src=src, ld_src=ld_src, Rs=Rs, Cs=Cs, rowmap=rowmap, dst=dst, ld_dst=dst.shape[1], Rd=dst.shape[0],
                               Cd=n_rows_logical if transpose else dst.shape[1])
            capi.call('tfx_cast_rows_t' if transpose else 'tfx_cast_rows', a, stream)
        cast(w1, d, 2 * di, d, S['ff1'], rowmap=S['gmap'])
        cast(w1, d, 2 * di, d, S['ff1_t'], rowmap=S['gmap'], transpose=True, n_rows_logical=2 * dip)
        cast(w2, di, d, di, S['ff2'])
        cast(w2, di, d, di, S['ff2_t'], transpose=True, n_rows_logical=d)
        capi.check(capi.lib().tfx_gather_f32(b1.data_ptr(), S['gmap'].data_ptr(), S['ff1b'].data_ptr(), 2 * dip, ctypes.c_void_p(stream)), 'tfx_gather_f32')
        self._ver = ver

    def _buffers(self, T, dev):
        B = self.bufs.get(T)
        if B is None or B['hn'].device != dev:
            d, dip = self.d, self.dip
            e = lambda *s, dtype=BF16: torch.empty(*s, device=dev, dtype=dtype)
            self.bufs.clear()                                                         # one row count at a time: the buffers are activations of a step
            B = self.bufs[T] = dict(hn=e(T, d), ag=e(T, 2 * dip), hm=e(T, dip), pred=e(T, d), dpred=torch.zeros(T, d, device=dev, dtype=BF16),
                                    dag=e(T, 2 * dip), dhn=e(T, d), acc=torch.zeros(1, device=dev, dtype=torch.float32))
        return B

    def forward(self, x_ptr, T, dev, stream):
        """pred = FeedForward(RMSNorm(x)) for the T rows at x_ptr ([T, d] bf16)"""
        self._refresh(stream)
        B, S, E = self._buffers(T, dev), self.shadows, capi.ENUMS
        d, dip = self.d, self.dip
        gamma, _, _, _, b2 = self.params()
        self._x = x_ptr
        capi.call('tfx_rmsnorm_fwd', capi.make_args('tfx_rmsnorm_args', T=T, d=d, x=x_ptr, y=B['hn'], gamma=gamma), stream)
        capi.call('tfx_gemm_nt', capi.make_args('tfx_gemm_nt_args', A=B['hn'], lda=d, B=S['ff1'], ldb=d, M=T, N=2 * dip, K=d, epi=E['TFX_EPI_GEGLU'],
                                                C=B['ag'], ldc=2 * dip, C2=B['hm'], ldc2=dip, bias=S['ff1b']), stream)
        capi.call('tfx_gemm_nt', capi.make_args('tfx_gemm_nt_args', A=B['hm'], lda=dip, B=S['ff2'], ldb=dip, M=T, N=d, K=dip, epi=E['TFX_EPI_BF16'],
                                                C=B['pred'], ldc=d, bias=b2), stream)
        return B

    def backward(self, T, dx, stream):
        """from dpred (the head's work buffer, [T, d] bf16): the five parameter gradients (fresh fp32 tensors) and dx = d loss / d (head input) -> `dx`"""
        B, S, E = self.bufs[T], self.shadows, capi.ENUMS
        d, di, dip = self.d, self.di, self.dip
        gamma, w1, b1, w2, b2 = self.params()
        g = [torch.zeros_like(p) for p in (gamma, w1, b1, w2, b2)]
        sp = ctypes.c_void_p(stream)
        lib = capi.lib()
        tn = lambda **kw: capi.call('tfx_gemm_tn', capi.make_args('tfx_gemm_tn_args', M=T, splits=0, accumulate=1, alpha=1.0, **kw), stream)
        capi.check(lib.tfx_colsum_bf16(B['dpred'].data_ptr(), d, T, d, None, None, g[4].data_ptr(), sp), 'tfx_colsum_bf16')
        tn(N=d, K=di, k_valid=di, A=B['dpred'], lda=d, a_cols=d, B=B['hm'], ldb=dip, b_cols=dip, C=g[3], ldc=di)
        capi.call('tfx_gemm_nt', capi.make_args('tfx_gemm_nt_args', A=B['dpred'], lda=d, B=S['ff2_t'], ldb=d, M=T, N=dip, K=d, epi=E['TFX_EPI_GEGLU_BWD'],
                                                C=B['dag'], ldc=2 * dip, aux=B['ag'], ldaux=2 * dip), stream)
        tn(N=2 * dip, K=d, k_valid=d, A=B['dag'], lda=2 * dip, a_cols=2 * dip, B=B['hn'], ldb=d, b_cols=d, rowmap=S['gmap'], C=g[1], ldc=d, colsum=g[2])
        capi.call('tfx_gemm_nt', capi.make_args('tfx_gemm_nt_args', A=B['dag'], lda=2 * dip, B=S['ff1_t'], ldb=2 * dip, M=T, N=d, K=2 * dip,
                                                epi=E['TFX_EPI_BF16'], C=B['dhn'], ldc=d), stream)
        capi.call('tfx_rmsnorm_bwd', capi.make_args('tfx_rmsnorm_args', T=T, d=d, x=self._x, gamma=gamma, dy=B['dhn'], dx=dx, dgamma=g[0]), stream)
        return g


class _HeadCosine(torch.autograd.Function):
    """default path: head forward + fused cosine loss as native launches behind the student's step; the backward scales the loss seed by the
    upstream gradient (as the fused step scales its seeds), runs the head's backward and hands d loss / d hidden back as a view of the tap's buffer"""

    @staticmethod
    def forward(ctx, wrapper, hidden, target_ptr, geom, *params):
        b, n, n_true, tap = geom
        head, stream = wrapper._head, wrapper.student._stream()
        T = b * n
        B = head.forward(hidden.data_ptr(), T, hidden.device, stream)
        B['acc'].zero_()
        capi.call('tfx_cosine_fwd_bwd', capi.make_args('tfx_cosine_args', T=T, d=head.d, pred=B['pred'], ld_pred=head.d, target=target_ptr, ld_target=head.d,
                                                       n_pad=n, n_valid=n_true, grad_scale=1.0 / (b * n_true), dpred=B['dpred'], ld_d=head.d, acc=B['acc']), stream)
        ctx.wrapper, ctx.geom, ctx.step = wrapper, geom, wrapper._step
        return 1. - B['acc'][0] / (b * n_true)

    @staticmethod
    def backward(ctx, grad_rep):
        wrapper = ctx.wrapper
        b, n, n_true, tap = ctx.geom
        if ctx.step != wrapper._step:
            raise RuntimeError('backward() of a stale loss: the prediction head keeps the activations of the latest forward only')
        head, stream = wrapper._head, wrapper.student._stream()
        T = b * n
        go = grad_rep.reshape(()).to(torch.float32)
        dpred = head.bufs[T]['dpred']
        capi.check(capi.lib().tfx_scale_bf16_dev(dpred.data_ptr(), dpred.numel(), go.data_ptr(), ctypes.c_void_p(stream)), 'tfx_scale_bf16_dev')
        g = head.backward(T, tap.data_ptr(), stream)
        return (None, tap[:, :n_true], None, None, *g)


class _HeadPred(torch.autograd.Function):
    """custom `loss_fn`: the head's output leaves as a (b, n, dim) fp32 tensor, the callable's gradient comes back into the native backward"""

    @staticmethod
    def forward(ctx, wrapper, hidden, geom, *params):
        b, n, n_true, tap = geom
        head, stream = wrapper._head, wrapper.student._stream()
        B = head.forward(hidden.data_ptr(), b * n, hidden.device, stream)
        ctx.wrapper, ctx.geom, ctx.step = wrapper, geom, wrapper._step
        return B['pred'].view(b, n, head.d)[:, :n_true].float()

    @staticmethod
    def backward(ctx, grad_pred):
        wrapper = ctx.wrapper
        b, n, n_true, tap = ctx.geom
        if ctx.step != wrapper._step:
            raise RuntimeError('backward() of a stale loss: the prediction head keeps the activations of the latest forward only')
        head, stream = wrapper._head, wrapper.student._stream()
        T = b * n
        dpred = head.bufs[T]['dpred'].view(b, n, head.d)
        if n_true < n:
            dpred[:, n_true:].zero_()
        dpred[:, :n_true].copy_(grad_pred)
        g = head.backward(T, tap.data_ptr(), stream)
        return (None, tap[:, :n_true], None, *g)


class SelfMaskedRepTraining(nn.Module):
    def __init__(self, net, ema_beta=0.999, rep_loss_weight=0.1, student_layer=-3, teacher_layer=-1, loss_fn=default_rep_loss_fn,
                 use_asymmetric_dropout=True, student_dropout_rate=0.1, teacher_dropout_rate=0.):
        from .lora import require_no_lora
        require_no_lora(net, 'SelfMaskedRepTraining')
        super().__init__()
        assert not use_asymmetric_dropout or student_dropout_rate > teacher_dropout_rate, 'student must have greater dropout rate than teacher to ensure teacher has a better view'
        if use_asymmetric_dropout:
            raise NotImplementedError('SelfMaskedRepTraining(use_asymmetric_dropout=True): the MI355X kernels have no dropout (Transformer(dropout=...) raises too), '
                                      'so switching dropout probabilities would train something else without saying so - pass use_asymmetric_dropout=False '
                                      '(teacher = EMA weights, its own noise, a deeper layer)')
        if rep_loss_weight > 0 and not engine.pull_form_ok(net.md):
            raise NotImplementedError('SelfMaskedRepTraining needs hidden taps, which ride on the pull-form AttentionResidual backward '
                                      f'({engine.PULL_LIMITS}); this model has depth {net.md.depth}, dim {net.md.dim}')
        self.student = net
        self.teacher = net.create_ema(beta=ema_beta)
        self.rep_loss_weight = rep_loss_weight
        self.has_ssl_loss = rep_loss_weight > 0
        self.use_asymmetric_dropout = use_asymmetric_dropout
        self.student_dropout_rate, self.teacher_dropout_rate = student_dropout_rate, teacher_dropout_rate
        self.student_layer, self.teacher_layer = student_layer, teacher_layer
        self.loss_fn = loss_fn
        dim = net.dim
        self.student_predict_head = nn.Sequential(_HeadNorm(dim), _HeadFeedForward(dim))
        self.register_buffer('zero', torch.tensor(0.))
        self._head = _Head(self, dim)
        self._head_epoch = 0
        self.teacher_hiddens_only = True
        self._step = 0
        if next(net.parameters()).is_cuda:
            self.student_predict_head.to(next(net.parameters()).device); self.zero = self.zero.to(next(net.parameters()).device)

    # ------------------------------------------------------------------ the reference's surface
    def parameters(self, recurse=True):                                 # T:3507-3511
        return chain(self.student.parameters(), self.student_predict_head.parameters())

    def update_teacher(self):
        self.teacher.update()

    def mark_weights_changed(self):
        """the head's weights were edited where nothing can see it (in place through `.data`): rebuild its bf16 shadows on the next call; the student's too"""
        self._head_epoch += 1
        self.student.mark_weights_changed()

    # ------------------------------------------------------------------ what optim.FusedAdam / FusedMuon read
    def head_parameters(self):
        return list(self.student_predict_head.parameters())

    def muon_parameters(self):
        return self.student.muon_parameters()                            # the head is not in the reference's list (T:1657-1672)

    # ------------------------------------------------------------------ forward
    def forward(self, *args, **kwargs):
        batch = args[0] if args else kwargs.get('modalities')
        if torch.is_tensor(batch) or not isinstance(batch, (list, tuple)):
            raise NotImplementedError('SelfMaskedRepTraining runs on the list-of-samples form of Transfusion.forward (the tensor forms return no times, '
                                      'in the reference as well)')
        student, ema = self.student, self.teacher.ema_model
        md = student.md
        nh = md.depth + 2
        ks, kt = self.student_layer % nh, self.teacher_layer % nh
        if not self.has_ssl_loss:                                        # T:3533-3534
            student_loss, _ = student(*args, return_loss=True, return_times=True, **kwargs)
            return student_loss, (student_loss, self.zero)
        self._step += 1
        student_loss, student_hiddens, times, (splan, n_true) = student(*args, return_loss=True, return_hiddens=(ks,), return_times=True,
                                                                        _hidden_request=dict(raw=True), **kwargs)
        b, n = splan.b, splan.n
        hidden = student_hiddens[ks]                                     # (b, n_true, d) bf16 view of the plan's rows, with the autograd edge of the step

        tkw = {k: v for k, v in kwargs.items() if k != 'times'}
        # the teacher needs its hiddens and nothing for a backward: a plan that keeps the hiddens alone (`teacher_hiddens_only = False`: a full training plan)
        with torch.no_grad():
            _, teacher_hiddens, (tplan, _) = ema(*args, times=times, return_loss=True, return_hiddens=(kt,),
                                                 _hidden_request=dict(raw=True, hiddens_only=self.teacher_hiddens_only), **tkw)
        self._teacher_plan = tplan
        if (tplan.b, tplan.n) != (b, n):
            raise capi.TfxError('student and teacher packed the batch differently')
        geom = (b, n, n_true, splan.tap_buffer(ks))
        params = _head_params(self.student_predict_head)
        if not hidden.requires_grad:                                     # under no_grad: values only
            hidden = hidden.detach()
        if self.loss_fn is default_rep_loss_fn:
            target = tplan.embed if kt == md.depth + 1 else tplan.hid[kt]
            rep = _HeadCosine.apply(self, hidden, target.data_ptr(), geom, *params)
        else:
            pred = _HeadPred.apply(self, hidden, geom, *params)
            rep = self.loss_fn(pred, teacher_hiddens[kt].float())
        total = student_loss + rep * self.rep_loss_weight
        return total, (student_loss, rep)
