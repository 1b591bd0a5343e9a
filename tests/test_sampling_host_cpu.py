"""The host side of `sample_many` (transfusion_pytorch_amd/sampling.py), none of which needs a GPU or the library: the row layouts of a step of the continuous
schedule against tests/_sampling_cases.py's per-row restatement, the solver control block against the tableaus, and the per-sample state machine driven by
scripted token streams against hand-written counters."""
import os
import sys
from fractions import Fraction as Fr
from types import SimpleNamespace

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _ode_rk_cases as RK                                                                  # noqa: E402
import _sampling_cases as C                                                                 # noqa: E402
from transfusion_pytorch_amd import ode, sampling                                           # noqa: E402
from transfusion_pytorch_amd.sampling import Sampler, _Call, compact_layout, dense_layout, step_roles    # noqa: E402

ARRAYS = ('ids', 'pos', 'kve', 'rot', 'tok_inst', 'blk_rows', 'row_ty', 'unit_row0')


# ---------------------------------------------------------------------------------------------- 1. layouts
def test_the_mirror_rows_are_the_ones_the_cases_name():
    assert [getattr(sampling, n) for n in ('PH', 'CL', 'UL', 'TS', 'UP', 'LT', 'LL', 'TY', 'OK', 'SP', 'CP')] == [C.F[n] for n in C.FIELDS]


def live_rows(lay, Lq=None):
    """{(unit, id, pos, kve, rot, instance)} over the rows that write a cache position"""
    pos = np.asarray(lay['pos']).reshape(-1)
    if Lq is not None:
        unit = np.arange(pos.size) // Lq
    else:
        U = lay['unit_row0'].size
        unit = np.searchsorted(np.asarray(lay['units'][:U]) + np.asarray(lay['units'][U:2 * U]), np.arange(pos.size), side='right')
    flat = [np.asarray(lay[k]).reshape(-1) for k in ('ids', 'pos', 'kve', 'rot', 'tok_inst')]
    return sorted((int(unit[n]), *(int(a[n]) for a in flat)) for n in np.flatnonzero(pos >= 0))


def check_step(A, H, n_t, Lc, cap, bucket):
    """both layouts of one step against the reference, array for array, plus the two invariants; returns whether the step was mixed"""
    mixed = C.is_mixed(A)
    Lq = Lc + 1 if mixed else 1
    r = step_roles(A, H, n_t, C.NULL_ID)
    got, want = dense_layout(r, Lq, cap)._asdict(), C.reference_dense(A, H, n_t, Lq, cap)
    assert got['units'] is None and got['ids'].shape == (H, A.shape[1], Lq)
    for k in ARRAYS:
        assert np.array_equal(np.asarray(got[k]).reshape(-1), want[k].reshape(-1)), f'dense {k}'
    rows = live_rows(got, Lq)
    assert len({row[2] for row in rows}) == len(rows), 'a cache position is written twice'
    if mixed:                                                     # (only mixed steps are ever compacted)
        gotc, wantc = compact_layout(r, bucket, cap)._asdict(), C.reference_compact(A, H, n_t, bucket, cap)
        for k in ARRAYS + ('units',):
            assert np.array_equal(np.asarray(gotc[k]), wantc[k]), f'compacted {k}'
        assert live_rows(gotc) == rows, 'the two layouts carry different rows'
    return mixed


def test_layouts_equal_the_per_row_restatement_on_random_mirrors():
    rng = np.random.default_rng(20250)
    n_mixed = 0
    for _ in range(2000):
        A, H, n_t, Lc, cap = C.random_mirror(rng)
        n_mixed += check_step(A, H, n_t, Lc, cap, bucket=int(rng.choice([4, 8, 128])))
    assert n_mixed >= 1500, n_mixed


@pytest.mark.parametrize('case', C.edge_mirrors(), ids=lambda c: c[0])
def test_layouts_equal_the_per_row_restatement_on_edge_mirrors(case):
    name, A, H, n_t, Lc, cap, bucket = case
    mixed = check_step(A, H, n_t, Lc, cap, bucket)
    assert mixed == (name != 'not a mixed step (Lq = 1)')
    if 'bucket' in name:
        Tb = compact_layout(step_roles(A, H, n_t, C.NULL_ID), bucket, cap).ids.size
        assert Tb == (bucket if 'exactly' in name else 2 * bucket)


# ---------------------------------------------------------------------------------------------- 2. solver control block
@pytest.mark.parametrize('S', [2, 3, 16])
@pytest.mark.parametrize('method', ode.METHODS)
def test_solver_control_block_equals_the_tableau_restatement(method, S):
    order, c, A, b = RK.TABLEAUS[method]
    f32 = lambda x: np.float32(float(x))
    ts = torch.linspace(0, 1, S)
    times, modes, rows = [], [], []
    for k in range(S - 1):
        t0, t1, dt = float(ts[k]), float(ts[k + 1]), float(ts[k + 1] - ts[k])
        for q in range(len(c)):
            times.append(t1 if c[q] == 1 else t0 + float(c[q]) * dt)
            modes.append(2. if q == len(c) - 1 else 1.)
            wa = [f32(Fr(dt) * a) for a in A[q]] + [0.] * (3 - len(A[q]))
            wb = [f32(Fr(dt) * v) for v in b] + [0.] * (4 - len(b))
            rows.append([float(q), *wa, *wb])
    ctl = ode.ode_control(method, S)
    assert list(ctl.times) == times and all(type(t) is float for t in ctl.times)
    assert ctl.modes.dtype == np.float32 and ctl.modes.tolist() == modes
    assert ctl.rows.dtype == np.float32
    if method == 'midpoint':                                      # its own kernels take one coefficient: dt / 2 for the stage, dt for the step end
        dts = [float(ts[k + 1] - ts[k]) for k in range(S - 1)]
        want = np.array([[v for dt in dts for v in (dt * 0.5, dt)]], np.float32)
        assert ctl.rows.shape == want.shape and np.array_equal(ctl.rows.view(np.int32), want.view(np.int32))
    else:
        want = np.array(rows, np.float32).T
        assert ctl.rows.shape == (8, len(times)) and np.array_equal(ctl.rows.view(np.int32), want.view(np.int32))


# ---------------------------------------------------------------------------------------------- 3. state machine
S_, EOS, META, SOM, EOM = 100, 101, 102, [110, 111], [120, 121]
COUNTERS = ('cache_len', 'tokens_seen', 'num_tokens', 'uncond_len', 'uncond_pos', 'num_past_modalities', 'phase', 'unfed', 'som_pending', 'commit_pending')
N_EVALS = 2


def sampler():
    """a Sampler over a stub that carries the ids and shape tables the transitions read (type 0: default shape (4,), type 1: (3, 3))"""
    model = SimpleNamespace(device='cpu', md=None, sos_id=S_, eos_id=EOS, meta_id=META, som_ids=SOM, eom_ids=EOM, null_text_id=130,
                            modality_default_shape=[(4,), (3, 3)], modality_num_dim=[1, 2], fallback_to_default_shape_if_invalid=False,
                            to_modality_shape_fn=[lambda s: tuple(int(v) for v in s.split(','))] * 2)
    return Sampler(model)


def call(max_length, guided):
    return _Call(B=1, H=2 if guided else 1, use_cfg=guided, stream=0, max_length=max_length, temperature=0., min_p=0., fixed_shape=None, init_noise=None,
                 modality_steps=2, cfg_scale=3. if guided else 1.)


class Run:
    """one sample driven the way the loops drive it.  `lockstep`: the continuous schedule under guidance (the null-text cache is prefilled after the first
    token and then advances with every step); otherwise the phased schedule, whose null-text counters move between phases only"""

    def __init__(self, prompt, max_length, lockstep, force=None):
        self.smp, self.c, self.lockstep = sampler(), call(max_length, lockstep), lockstep
        self.st, = self.smp._initial_states([[prompt]], force)           # one prompt of one text part
        self.smp._maybe_transition(self.st, None)
        self.first = True

    def text(self, tok):
        st = self.st
        assert st.phase == 'text'
        if not self.first:                                        # (the prefill's token: everything before it is in the caches already)
            st.fed(self.lockstep)
        if st.accept(tok, EOS, self.c.max_length):
            self.smp._maybe_transition(st, self.c.fixed_shape)
        if self.first and self.lockstep:
            st.null_prefilled([p for p in st.parts[:-1] + [st.parts[-1][:-1]] if len(p)])
        self.first = False
        return self

    def block(self):
        st = self.st
        assert st.phase == 'modality'
        if self.first and self.lockstep:
            self.first = False
            st.budget(self.c.max_length)
            st.null_prefilled(st.parts)
        st.begin_block(self.lockstep)
        for _ in range(N_EVALS):
            if st.som_pending:
                st.som_fed()
            st.ode_k += 1
        st.commit('BLOCK', EOM[st.curr_modality_id], self.c.max_length, self.lockstep)
        return self

    def check(self, parts, **counters):
        assert self.st.parts == parts
        assert self.st.curr_seq is self.st.parts[-1], 'the text being built is the last part'
        assert {k: getattr(self.st, k) for k in COUNTERS} == counters
        return self


def test_eos_as_the_first_token_ends_the_sample():
    for lockstep in (False, True):
        Run([7, 8], 20, lockstep).text(EOS).check(
            [[S_, 7, 8, EOS]], cache_len=3, tokens_seen=3, num_tokens=1, uncond_len=3 * lockstep, uncond_pos=3 * lockstep, num_past_modalities=0, phase='done', unfed=True,
            som_pending=False, commit_pending=False)


@pytest.mark.parametrize('tok', [5, SOM[1]])
def test_max_length_0_accepts_one_token_and_opens_nothing(tok):
    r = Run([7, 8], 0, False).text(tok).check([[S_, 7, 8, tok]], cache_len=3, tokens_seen=3, num_tokens=1, uncond_len=0, uncond_pos=0, num_past_modalities=0, phase='done',
                                              unfed=True, som_pending=False, commit_pending=False)
    assert r.st.modality_length is None


def test_max_length_1_accepts_two_tokens():
    r = Run([7, 8], 1, False).text(5)
    assert r.st.phase == 'text'
    r.text(6).check([[S_, 7, 8, 5, 6]], cache_len=4, tokens_seen=4, num_tokens=2, uncond_len=0, uncond_pos=0, num_past_modalities=0, phase='done', unfed=True,
                    som_pending=False, commit_pending=False)


@pytest.mark.parametrize('lockstep', [False, True])
def test_som_with_the_default_shape_then_commit_then_text(lockstep):
    """[som] of type 1 sampled second: the default shape (3, 3), a block of 9.  The real cache never takes the [som] (T:2411), the null-text cache does; under
    lock-step the committed block enters the null-text cache with the [eom] that follows it (the `commit_pending` catch-up)"""
    r = Run([7, 8], 20, lockstep).text(5).text(SOM[1])
    st = r.st
    assert (st.phase, st.curr_modality_id, st.modality_shape, st.modality_length) == ('modality', 1, (3, 3), 9)
    null = lambda n: n if lockstep else 0
    r.check([[S_, 7, 8, 5, SOM[1]]], cache_len=4, tokens_seen=4, num_tokens=2, uncond_len=null(4), uncond_pos=null(4), num_past_modalities=0, phase='modality', unfed=True,
            som_pending=False, commit_pending=False)
    st.begin_block(lockstep)
    assert st.som_pending == lockstep and st.ode_k == 0
    r.block().check([[S_, 7, 8, 5, SOM[1]], 'BLOCK', [EOM[1]]], cache_len=13, tokens_seen=5, num_tokens=11, uncond_len=null(5), uncond_pos=null(5), num_past_modalities=1,
                    phase='text', unfed=True, som_pending=False, commit_pending=lockstep)
    assert st.last_token == EOM[1] and st.ode_k == N_EVALS
    r.text(9).check([[S_, 7, 8, 5, SOM[1]], 'BLOCK', [EOM[1], 9]], cache_len=14, tokens_seen=6, num_tokens=12, uncond_len=null(15), uncond_pos=null(7), num_past_modalities=1,
                    phase='text', unfed=True, som_pending=False, commit_pending=False)


@pytest.mark.parametrize('max_length,phase', [(10, 'text'), (9, 'done')])
def test_max_length_exactly_reached_by_a_block(max_length, phase):
    """1 token + a block of 9 = 10 decoded tokens: a budget of 10 is reached, not passed - the sample goes on to one more token; a budget of 9 ends it at the commit"""
    r = Run([7], max_length, True).text(SOM[1]).block()
    r.check([[S_, 7, SOM[1]], 'BLOCK', [EOM[1]]], cache_len=11, tokens_seen=3, num_tokens=10, uncond_len=3, uncond_pos=3, num_past_modalities=1, phase=phase, unfed=True,
            som_pending=False, commit_pending=phase == 'text')
    if phase == 'text':
        r.text(4).check([[S_, 7, SOM[1]], 'BLOCK', [EOM[1], 4]], cache_len=12, tokens_seen=4, num_tokens=11, uncond_len=13, uncond_pos=5, num_past_modalities=1, phase='done',
                        unfed=True, som_pending=False, commit_pending=False)


def test_som_with_meta_shape_tokens():
    five = META + 1 + ord('5')
    r = Run([7], 20, False).text(META).text(five).text(SOM[0])
    assert (r.st.phase, r.st.curr_modality_id, r.st.modality_shape, r.st.modality_length) == ('modality', 0, (5,), 5)
    r.block().check([[S_, 7, META, five, SOM[0]], 'BLOCK', [EOM[0]]], cache_len=9, tokens_seen=5, num_tokens=8, uncond_len=0, uncond_pos=0, num_past_modalities=1, phase='text',
                    unfed=True, som_pending=False, commit_pending=False)


@pytest.mark.parametrize('force,shape,prompt_tail', [(0, (4,), [SOM[0]]), ((1, (2, 2)), (2, 2), [META, META + 1 + ord('2'), META + 1 + ord(','), META + 1 + ord('2'), SOM[1]])])
def test_forced_modality_at_the_start(force, shape, prompt_tail):
    """the forced [som] (and its meta tokens) is part of the prompt: it went through the prefill of both caches, so no [som] is pending under lock-step"""
    r = Run([7], 20, True, force=force)
    st, n = r.st, 2 + len(prompt_tail)
    assert (st.phase, st.modality_shape, st.unfed) == ('modality', shape, False)
    L, ty = int(np.prod(shape)), st.curr_modality_id
    r.block().check([[S_, 7, *prompt_tail], 'BLOCK', [EOM[ty]]], cache_len=n + L, tokens_seen=n + 1, num_tokens=L, uncond_len=n, uncond_pos=n, num_past_modalities=1, phase='text',
                    unfed=True, som_pending=False, commit_pending=True)
    r.text(3).check([[S_, 7, *prompt_tail], 'BLOCK', [EOM[ty], 3]], cache_len=n + L + 1, tokens_seen=n + 2, num_tokens=L + 1, uncond_len=n + L + 1, uncond_pos=n + 2,
                    num_past_modalities=1, phase='text', unfed=True, som_pending=False, commit_pending=False)
