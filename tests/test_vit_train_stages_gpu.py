"""The fine-tuning backward pass (csrc/vit_train.hip, csrc/attention_bwd.hip) stage by stage, element by element,
against the float64 restatements of tests/vit_train_ref.py, with each element's error bound derived there.

Each stage of a 2-block tower runs on its own (``VisualTower.backward(stages=...)``); what it reads (the tape, the
entry dx / dx16, the 16-bit weight copies) and what it leaves (dx, dx16, dq | dk | dv, da16, dh32, delta) are read
back through ``ec_vit_train_layout``, so a stage is checked on exactly the inputs it consumed.  The shapes are the
shipped fine-tuning batches of ViT-B/16 and ViT-L/14 and the row counts that reach the host-side branches
(tests/test_vit_train_cpu.py asserts which).  d_feats = feats (the gradient of |f|^2 / 2): the class rows' gradient
is then correlated with their LayerNorm output, so every term of the LayerNorm backward carries weight.  Every
gradient buffer starts as NaN."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vit_train_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

EMBED = {'B/16': 512, 'L/14': 768, 'L/14@336': 768, 'wide_odd': 32, 'tiny': 16}
STAGE_RUNS = [('b16_n32', 'float16'), ('b16_n32', 'bfloat16'), ('b16_n128', 'float16'), ('l14_n32', 'float16'),
              ('l14_n64', 'float16'), ('l14_336_n2', 'float16'), ('wide_odd_n9', 'float16'), ('tiny_n5', 'float16')]


def _assert_within(got, want, bound, what=''):
    """Element by element |got - want| <= bound (NaN fails); reports the worst element."""
    got = got.reshape(want.shape)
    err = (got.double() - want).abs()
    ok = err <= bound
    if not bool(ok.all()):
        ratio = torch.where(ok, torch.zeros_like(err), (err / bound).nan_to_num(float('inf')))
        i = int(ratio.flatten().argmax())
        idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), err.shape))
        raise AssertionError(f'{what}: {int((~ok).sum())} of {err.numel()} elements outside the bound; worst at {idx}: '
                             f'got {float(got.flatten()[i]):.8g} want {float(want.flatten()[i]):.8g} '
                             f'err {float(err.flatten()[i]):.3g} bound {float(bound.flatten()[i]):.3g}')


def _cfg(case):
    arch = ref.CASES[case][0]
    R, P, W = ref.ARCH[arch]
    return dict(image_size=R, patch=P, width=W, layers=2, embed_dim=EMBED[arch], text_width=64, text_heads=1,
                text_layers=1, context_length=77, vocab_size=128)


def _tower(case, dtype, seed=0):
    from eventclip_amd import clip as eclip, ft
    cfg = _cfg(case)
    sd = eclip.random_state_dict(cfg, seed=seed)
    model = eclip.CLIP(cfg, sd, dtype=dtype, full_last_block=True, ln_folded=False, q_scaled=False).cuda()
    return model, ft.VisualTower(model)


def _patches(tower, n, seed):
    from eventclip_amd import _lib
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, 3, tower.cfg['image_size'], tower.cfg['image_size'], generator=g).cuda()
    patches = torch.empty((n, tower.G, tower.kpad), dtype=tower.cd, device='cuda')
    _lib.check(_lib.lib().ec_patchify(_lib.ptr(x), n, tower.cfg['image_size'], tower.P, tower.kpad, _lib.ptr(patches),
                                      tower.code, _lib.stream_ptr()), 'ec_patchify')
    return patches


def _block(tower, l):
    from eventclip_amd import ft
    w16 = {f: tower.packed[(l, f)] for f in ft._MATRICES}
    master = {f: tower.master[ft._block_name(l, leaf)] for f, leaf in ft._BLOCK}
    return w16, master


@pytest.fixture(scope='module', params=STAGE_RUNS, ids=[f'{c}-{d}' for c, d in STAGE_RUNS])
def run(request, hip):
    """Forward over the case's batch, then every stage of the backward one call at a time; the workspace state
    after each stage is kept."""
    case, dtype = request.param
    model, tower = _tower(case, dtype)
    n = ref.CASES[case][1]
    patches = _patches(tower, n, seed=1)
    feats = tower.forward(patches)
    d_feats = feats.clone()
    want = tower.canonical(list(tower.master))
    _, views, flat, _ = tower._grad_struct(want)
    flat.fill_(float('nan'))
    top, blocks = tower.workspace_views(n)
    M, W = n * tower.S, tower.W
    states = []
    for j in range(tower.L + 2):
        tower.backward(d_feats, want, stages=(j, j + 1))
        st = {k: top[k].clone() for k in ('dx', 'dx16', 'dh32', 'da16', 'delta', 'clsln', 'dclsln')}
        st['dqkv'] = top['g16'].reshape(-1)[:M * 3 * W].view(M, 3 * W).clone()
        states.append(st)
    torch.cuda.synchronize()
    yield dict(case=case, dtype=getattr(torch, dtype), tower=tower, n=n, patches=patches, d_feats=d_feats, top=top,
               blocks=blocks, states=states, grads=views, flat=flat, want=want)
    del tower, model
    torch.cuda.empty_cache()


def test_every_gradient_is_written_and_finite(run):
    assert bool(torch.isfinite(run['flat'][:sum(v.numel() for v in run['grads'].values())]).all())


def test_forward_tape(run):
    """x[l + 1], xm[l], u[l], gact[l] and lse[l] against float64 of the tape's own inputs (at M = 16448 the
    c_proj GEMM's last 64 rows go through gemm_rows32's K-batched tail and tail_fixup_kernel)."""
    t, dt, n = run['tower'], run['dtype'], run['n']
    for l, tape in enumerate(run['blocks']):
        w16, master = _block(t, l)
        r = ref.block_forward(tape, w16, master, dt, n, t.S, t.W // 64)
        nxt = run['blocks'][l + 1]['x'] if l + 1 < t.L else run['top']['x_last']
        _assert_within(tape['xm'], *r['xm'], what=f'block {l} xm')
        _assert_within(tape['u'], *r['u'], what=f'block {l} u')
        _assert_within(tape['gact'], *r['gact'], what=f'block {l} gact')
        _assert_within(nxt, *r['x_next'], what=f'block {l} x[l + 1]')
        _assert_within(tape['lse'], *r['lse'], what=f'block {l} lse')


def test_head_stage(run):
    t, dt, n = run['tower'], run['dtype'], run['n']
    st = run['states'][0]
    r = ref.head_backward(run['top']['x_last'], st['clsln'], st['dclsln'], run['d_feats'], t.master, n, t.S, dt)
    _assert_within(st['clsln'], *r['clsln'], what='clsln')
    _assert_within(st['dclsln'], *r['dclsln'], what='dclsln')
    for k in ('proj', 'ln_post.weight', 'ln_post.bias'):
        _assert_within(run['grads'][k], *r[k], what=k)
    _assert_within(st['dx'], *r['dx'], what='dx')
    _assert_within(st['dx16'], *r['dx16'], what='dx16')


@pytest.mark.parametrize('stage', [1, 2])
def test_block_stage(run, stage):
    from eventclip_amd import ft
    t, dt, n = run['tower'], run['dtype'], run['n']
    l = t.L - stage
    entry, st = run['states'][stage - 1], run['states'][stage]
    w16, master = _block(t, l)
    r = ref.block_backward(run['blocks'][l], entry['dx'], entry['dx16'], w16, master, dt, n, t.S, t.W // 64)
    for f, leaf in ft._BLOCK:
        _assert_within(run['grads'][ft._block_name(l, leaf)], *r[f], what=f'block {l} {leaf}')
    _assert_within(st['da16'], *r['da16'], what=f'block {l} da16')
    _assert_within(st['dqkv'], *r['g16'], what=f'block {l} dq | dk | dv')
    _assert_within(st['delta'], *r['delta'], what=f'block {l} delta')
    _assert_within(st['dh32'], *r['dh32'], what=f'block {l} dh32')
    _assert_within(st['dx'], *r['dx'], what=f'block {l} exit dx')
    _assert_within(st['dx16'], *r['dx16'], what=f'block {l} exit dx16')


def test_embedding_stage(run):
    t, dt, n = run['tower'], run['dtype'], run['n']
    entry, st = run['states'][t.L], run['states'][t.L + 1]
    r = ref.embedding_backward(run['top']['pre'], entry['dx'], st['dh32'], run['patches'], t.master, n, t.S, t.k, dt)
    _assert_within(st['dh32'], *r['dh32'], what='d embedding (dh32)')
    for k in ('ln_pre.weight', 'ln_pre.bias', 'positional_embedding', 'class_embedding', 'conv1.weight'):
        _assert_within(run['grads'][k], *r[k], what=k)


# ---- LoRA factor gradients from the activations ----
@pytest.mark.parametrize('case,spec,dtype', [('tiny_n5', 'qkvo-4', 'float16'), ('wide_odd_n9', 'qkvo-16', 'float16'),
                                             ('wide_odd_n9', 'qkvo-24', 'float16'), ('tiny_n5', 'qkvo-64', 'float16'),
                                             ('wide_odd_n9', 'qkvo-64', 'bfloat16'), ('l14_n32', 'qkvo-16', 'float16'),
                                             ('b16_n32', 'qkvo-64', 'float16'), ('l14_336_n2', 'qkvo-24', 'float16'),
                                             # every rank next to a 16-row factor tile (RT = 1 .. 4) and the two- and
                                             # three-set sharing bodies, on the two smallest towers (M = 25, M = 90)
                                             ('tiny_n5', 'qv-1', 'float16'), ('tiny_n5', 'qkv-15', 'float16'),
                                             ('wide_odd_n9', 'qv-16', 'float16'), ('wide_odd_n9', 'qv-17', 'float16'),
                                             ('tiny_n5', 'qkvo-32', 'float16'), ('wide_odd_n9', 'qkvo-33', 'float16'),
                                             ('tiny_n5', 'qkv-40', 'float16'), ('wide_odd_n9', 'qkvo-48', 'float16'),
                                             ('tiny_n5', 'qkvo-49', 'float16'), ('tiny_n5', 'qkv-40', 'bfloat16')])
def test_lora_factor_gradients(hip, case, spec, dtype):
    """d up = dy^T (x down^T), d down = (dy up)^T x of block 0 (q, k, v: x = ln_1 output, dy = dq | dk | dv;
    out_proj: x = the attention output, dy = the 16-bit gradient of xm).  With only LoRA factors training, the pass
    stops after block 0's factor gradients, so g16 and dx16 still hold what they consumed."""
    from eventclip_amd import ft
    model, tower = _tower(case, dtype, seed=5)
    lf = ft.LoraFactors(tower, spec)
    torch.manual_seed(11)
    for k, p in lf.params.items():
        if 'lora_up' in k:
            p.copy_(torch.randn_like(p) * 0.02)
    grads = {k: torch.full_like(p, float('nan')) for k, p in lf.params.items()}
    lf.bind(grads)
    lf.merge()
    n = ref.CASES[case][1]
    feats = tower.forward(_patches(tower, n, seed=2))
    tower.backward(feats.clone(), [], lf.struct)
    torch.cuda.synchronize()
    top, blocks = tower.workspace_views(n)
    W, M, dt = tower.W, n * tower.S, getattr(torch, dtype)
    dqkv = top['g16'].reshape(-1)[:M * 3 * W].view(M, 3 * W)
    for i, j, kd, ku in lf.projections():
        assert torch.isfinite(grads[ku]).all() and torch.isfinite(grads[kd]).all(), ku
        if i != 0:
            continue
        x = blocks[0]['h1'] if j is not None else blocks[0]['att']
        dy = dqkv[:, j * W:(j + 1) * W] if j is not None else top['dx16']
        d_up, d_down = ref.lora_grads(x.double(), dy.double(), None, lf.down16[kd], lf.up16t[ku], lf.r, dt)
        _assert_within(grads[ku], *d_up, what=f'{ku}')
        _assert_within(grads[kd], *d_down, what=f'{kd}')


# ---- ec_attention_backward on its own ----
def _attention(qkv, n, S, W, heads):
    from eventclip_amd import _lib, ops
    out = torch.empty(n * S, W, device='cuda', dtype=qkv.dtype)
    lse = torch.empty(n, heads, S, device='cuda')
    _lib.check(_lib.lib().ec_attention_train(_lib.ptr(qkv), _lib.ptr(out), _lib.ptr(lse), n, S, W, heads,
                                             ops.dtype_code(qkv.dtype), _lib.stream_ptr()), 'ec_attention_train')
    return out, lse


@pytest.mark.parametrize('S,heads,n,dtype', [(50, 12, 2, 'float16'), (197, 12, 2, 'float16'), (197, 12, 2, 'bfloat16'),
                                             (257, 16, 2, 'float16'), (577, 16, 2, 'float16'), (1, 2, 3, 'float16'),
                                             (288, 2, 2, 'float16'), (289, 2, 2, 'float16')])
def test_attention_backward_per_element(hip, S, heads, n, dtype):
    """dq, dk, dv and delta against float64 of the same 16-bit q | k | v, output and dO and the kernel's own lse, at
    the towers' (S, heads) and at the edges of the 288-row staging (S = 1, 288, 289)."""
    from eventclip_amd import _lib, ops
    dt = getattr(torch, dtype)
    torch.manual_seed(S + heads)
    W = heads * 64
    qkv = (torch.randn(n * S, 3 * W, device='cuda') * 1.5).to(dt)
    out, lse = _attention(qkv, n, S, W, heads)
    dout = (torch.randn(n * S, W, device='cuda') * 0.5).to(dt)
    dqkv = torch.full_like(qkv, float('nan'))
    delta = torch.full((n, heads, S), float('nan'), device='cuda')
    _lib.check(_lib.lib().ec_attention_backward(_lib.ptr(qkv), _lib.ptr(out), _lib.ptr(lse), _lib.ptr(dout),
                                                _lib.ptr(dqkv), _lib.ptr(delta), n, S, W, heads, ops.dtype_code(dt),
                                                _lib.stream_ptr()), 'ec_attention_backward')
    g, eg, d, ed = ref.attention_backward(qkv.double(), out.double(), lse.double(), dout.double(), None, n, S, heads, dt)
    for j, name in enumerate(('dq', 'dk', 'dv')):
        _assert_within(dqkv[:, j * W:(j + 1) * W], g[:, j * W:(j + 1) * W], eg[:, j * W:(j + 1) * W], what=name)
    _assert_within(delta, d, ed, what='delta')
