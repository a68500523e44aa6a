"""Train-time augmentation in the loader's gather (a2m.data.Augment, PatsLoader.pairs(augment=),
csrc/augment.hip) on the device against its numpy restatement tests/augment_ref.py, bit for bit:
both kernels apply correctly rounded float32 operations in a fixed order, and numpy's float32
arithmetic is the same roundings.  The shapes are those of pats_data_ref at hop 5: N = 13 clips of
T = 64 frames (audio window 382, stride 6), here in batches of 5, 5 and 3."""
import functools

import numpy as np
import pytest
import torch

import augment_ref as R
import pats_data_ref as P
from test_gpu_validate import _trainer

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
ARR = P.arrays()
IDS = list('ABCD')
HOP, N, T = 5, 13, 64
ARENA, START, LAST = R.arena_tables(ARR, HOP)
SETTINGS = {
    # no magnitude is a power of two: r * t is then rounded, and a product fused with the sum that
    # follows it (one rounding instead of two) shows
    'tempo': dict(speed=0.45),
    'mirror+scale': dict(p_mirror=0.5, scale=0.3),
    'gain+masks': dict(gain=3., freq_mask=100, time_mask=20, mask_fill=-1.5),
}
SETTINGS['all'] = {k: v for s in list(SETTINGS.values()) for k, v in s.items()}
CONFIGS = dict(SETTINGS, off={})


def _table(datasets=('train',) * 4, ids=IDS):
    return [P.row(d, i, 'oliver') for d, i in zip(datasets, ids)]


def _loader(hop=HOP, shuffle=False, **kw):
    from a2m.data import PatsLoader
    kw.setdefault('table', _table())
    kw.setdefault('batch_size', 5)
    return PatsLoader(kw.pop('arrays', ARR), speaker='oliver', time=P.TIME, fs_new=P.FS_NEW, window_hop=hop,
                      shuffle=shuffle, device=DEV, **kw)


def _np(t):
    return t.detach().cpu().numpy()


def _stats(seed=11):
    """As test_gpu_data's: std[0] = std[52] = 1, one audio std entry below the 1e-7 guard."""
    g = np.random.default_rng(seed)
    pm = (g.standard_normal(104) * 30).astype(np.float32)
    ps = (g.random(104) * 50 + 5).astype(np.float32)
    pm[[0, 52]], ps[[0, 52]] = 0.0, 1.0
    am = (g.standard_normal(128) - 4).astype(np.float32)
    asd = (g.random(128) * 2 + 0.5).astype(np.float32)
    asd[5] = 1e-8
    return pm, ps, am, asd


PM, PS, AM, ASD = _stats()


def _dev(*a):
    return [torch.from_numpy(x).to(DEV) for x in a]


def _perm():
    from a2m.skeleton import mirror_permutation
    return np.asarray(mirror_permutation())


def _draw(cfg, pos, pass_, seed):
    s = CONFIGS[cfg]
    return R.draw(pos, pass_, seed=seed, p_mirror=s.get('p_mirror', 0.), speed=s.get('speed', 0.),
                  scale=s.get('scale', 0.), gain=s.get('gain', 0.), freq_mask=s.get('freq_mask', 0),
                  time_mask=s.get('time_mask', 0), C=128, T=T)


def _conditions(params):
    """What a parameter table of the 13 clips exercises, from the reference alone."""
    stretched = START[P.POSE] + np.floor(np.float32(63) * params[:, R.S]).astype(np.int64)      # row a of frame 63
    fw, f0, tw = params[:, R.FW], params[:, R.F0], params[:, R.TW]
    return {'mirrored': bool((params[:, R.MIRROR] == 1).any()), 'unmirrored': bool((params[:, R.MIRROR] == 0).any()),
            'clamped at the last row': bool((stretched > LAST[P.POSE]).any()),
            'mask at channel 0': bool(((fw > 0) & (f0 == 0)).any()),
            'mask ending at C': bool(((fw > 0) & (f0 + fw == 128)).any()),
            'zero-width mask': bool((fw == 0).any() or (tw == 0).any()),
            'time mask': bool((tw > 0).any())}


@functools.lru_cache(None)
def _seed():
    """The first seed whose pass 0 over the 13 clips holds every condition, chosen with the reference."""
    for seed in range(20000):
        if all(_conditions(_draw('all', np.arange(N), 0, seed)).values()):
            return seed
    raise AssertionError('no seed below 20000 holds every condition')


@functools.lru_cache(None)
def _reference(cfg, mode, pass_=0):
    """(params [13, 8], audio [13, 64, 128], pose [13, 64, 104]) of the clips 0..12; computed once a
    configuration and shared, never written to."""
    pos = np.arange(N)
    params = _draw(cfg, pos, pass_, _seed())
    fill = CONFIGS[cfg].get('mask_fill', 0.)
    a_mode, a_stats = (R.STANDARDISE, (AM, ASD)) if mode == 'norm' else (R.RAW, (None, None))
    audio = R.gather(ARENA[P.AUDIO], START[P.AUDIO], LAST[P.AUDIO], pos, 6, T, params, R.AUDIO, a_mode, *a_stats,
                     mask_fill=fill)
    if mode == 'raw':
        pose = R.gather(ARENA[P.POSE], START[P.POSE], LAST[P.POSE], pos, 1, T, params)
    else:
        pose = R.gather(ARENA[P.POSE], START[P.POSE], LAST[P.POSE], pos, 1, T, params, R.POSE, R.NECKSUB, PM, PS,
                        _perm())
    for x in (params, audio, pose):
        x.setflags(write=False)
    return params, audio, pose


def _augment(cfg, **kw):
    from a2m.data import Augment
    return Augment(seed=_seed(), **SETTINGS[cfg], **kw)


def _pairs(loader, mode, **kw):
    stats = {'norm': (PM, PS, AM, ASD), 'rawaudio': (PM, PS), 'raw': ()}[mode]
    return loader.pairs('train', *_dev(*stats), **kw)


def _bits(a, b):
    """Equal bit for bit (NaN-safe, and a -0 is not a +0)."""
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32),
                                                 np.ascontiguousarray(b).view(np.uint32))


# ------------------------------------------------------------------------------ the arithmetic
def test_the_chosen_seed_holds_every_condition():
    """From the reference: a mirrored and an unmirrored clip, a stretched read clamped at its interval's
    last row, a frequency mask at channel 0 and one ending at C = 128, a zero-width mask, a time mask.
    The device comparisons below run on exactly these tables."""
    params = _reference('all', 'norm')[0]
    got = _conditions(params)
    print(f'AUG seed {_seed()}: {got}')
    assert all(got.values()), got
    assert _conditions(_reference('tempo', 'norm')[0])['clamped at the last row']
    m = _conditions(_reference('mirror+scale', 'norm')[0])
    assert m['mirrored'] and m['unmirrored']
    k = _conditions(_reference('gain+masks', 'norm')[0])
    assert k['mask at channel 0'] and k['mask ending at C'] and k['zero-width mask'] and k['time mask']
    # the clamp is seen in the rows read: some clip reads its interval's last row more than once
    pos = int(np.argmax(START[P.POSE] + np.floor(np.float32(63) * params[:, R.S]).astype(np.int64) - LAST[P.POSE]))
    a, b, _ = R.rows_read(START[P.POSE][pos], LAST[P.POSE][pos], 1, T, params[pos, R.S])
    assert (b == LAST[P.POSE][pos]).sum() > 1 and (a == LAST[P.POSE][pos]).any() and a.max() == LAST[P.POSE][pos]


CASES = [(c, 'norm') for c in SETTINGS] + [(c, 'rawaudio') for c in SETTINGS] + [('tempo', 'raw'), ('gain+masks', 'raw')]


@pytest.mark.parametrize('cfg,mode', CASES, ids=[f'{c}-{m}' for c, m in CASES])
def test_augmented_pairs_equal_the_reference_bitwise(cfg, mode):
    """pairs(augment=) in batches of 5, 5 and 3: the drawn table (last_params) and both modalities of
    every batch, bit for bit; pose neck-subtracted with audio standardised ('norm') or raw
    ('rawaudio'), or both raw ('raw': tempo on the pose, no mirror or scale)."""
    params, audio, pose = _reference(cfg, mode)
    view = _pairs(_loader(), mode, augment=_augment(cfg), copy=True)
    assert len(view) == 3
    seen = 0
    for b0, (got_a, got_p) in zip((0, 5, 10), view):
        n = got_a.shape[0]
        assert n == (5, 5, 3)[b0 // 5] and got_p.shape == (n, T, 104) and got_a.shape == (n, T, 128)
        assert _bits(_np(view.last_params), params[b0:b0 + n]), (cfg, mode, b0)
        assert _bits(_np(got_a), audio[b0:b0 + n]), (cfg, mode, b0, 'audio')
        assert _bits(_np(got_p), pose[b0:b0 + n]), (cfg, mode, b0, 'pose')
        seen += n
    assert seen == N
    off = _reference('off', mode)                            # and the settings did act on what they name
    assert _bits(audio, off[1]) == (cfg == 'mirror+scale') and _bits(pose, off[2]) == (cfg == 'gain+masks')


def test_reversed_order_in_batches_of_three():
    """order= reversed, batch_size 3 (3, 3, 3, 3, 1): the parameters follow the clip, not its place."""
    params, audio, pose = _reference('all', 'norm')
    rev = np.arange(N)[::-1].copy()
    view = _pairs(_loader(batch_size=3), 'norm', augment=_augment('all'), copy=True, order=rev)
    got = list(view)
    assert [a.shape[0] for a, _ in got] == [3, 3, 3, 3, 1]
    assert _bits(_np(torch.cat([a for a, _ in got])), audio[rev])
    assert _bits(_np(torch.cat([p for _, p in got])), pose[rev])


def test_unit_speed_never_reads_the_next_row():
    """hop 0: one clip an interval (A, C, D), the windows disjoint.  Every row the plain gather does
    not read -- between the strided audio rows, after the clip, the interval's last -- is NaN.  A
    hand-made table with s = 1 and everything else active through gather_augmented stays finite and
    equals the reference: with a zero fraction row i + 1 is not touched."""
    from a2m.data import MODE_NECKSUB, MODE_STANDARDISE
    arr = {i: {m: np.full_like(a, np.nan) for m, a in mods.items()} for i, mods in ARR.items()}
    for i in IDS:
        arr[i][P.POSE][:64] = ARR[i][P.POSE][:64]
        arr[i][P.AUDIO][:382:6] = ARR[i][P.AUDIO][:382:6]
    loader = _loader(0, arrays=arr, batch_size=3)
    assert loader.index.size('train') == 3
    arena, start, last = R.arena_tables(arr, 0)
    assert np.isnan(arena[P.POSE][start[P.POSE] + 64]).all() and np.isnan(arena[P.AUDIO][start[P.AUDIO] + 1]).all()
    params = np.float32([[1, 1, 0.75, 2.5, 0, 7, 60, 4], [0, 1, 1.25, -1, 121, 7, 0, 0], [1, 1, 1, 0, 3, 0, 10, 1]])
    pm, ps, am, asd = _dev(PM, PS, AM, ASD)
    specs = [(P.AUDIO, MODE_STANDARDISE, am, asd), (P.POSE, MODE_NECKSUB, pm, ps)]
    order_dev = loader.upload('train', np.arange(3))
    got_a, got_p = loader.gather_augmented(order_dev, 0, 3, specs, _dev(params)[0], mask_fill=0.5)
    assert torch.isfinite(got_a).all() and torch.isfinite(got_p).all()
    pos = np.arange(3)
    want_a = R.gather(arena[P.AUDIO], start[P.AUDIO], last[P.AUDIO], pos, 6, T, params, R.AUDIO, R.STANDARDISE, AM, ASD,
                      mask_fill=0.5)
    want_p = R.gather(arena[P.POSE], start[P.POSE], last[P.POSE], pos, 1, T, params, R.POSE, R.NECKSUB, PM, PS, _perm())
    assert _bits(_np(got_a), want_a) and _bits(_np(got_p), want_p)
    assert (_np(got_a)[0, 60:] == 0.5).all() and (_np(got_a)[1, :, 121:] == 0.5).all()
    with pytest.raises(ValueError, match='params'):
        loader.gather_augmented(order_dev, 0, 3, specs, _dev(params[:2])[0])


# ------------------------------------------------------------------------------ identity and passes
@pytest.mark.parametrize('mode', ['norm', 'raw'])
def test_default_augment_is_the_identity(mode):
    from a2m.data import Augment
    loader = _loader()
    want = list(_pairs(loader, mode, copy=True))
    view = _pairs(loader, mode, augment=Augment(seed=9), copy=True)
    for _ in range(2):                                      # the pass number changes nothing either
        got = list(view)
        assert len(got) == len(want) == 3
        for (a, p), (wa, wp) in zip(got, want):
            assert _bits(_np(a), _np(wa)) and _bits(_np(p), _np(wp))


def test_passes_differ_and_a_new_view_repeats_them():
    """iter() k of a view draws for pass first_pass + k: two consecutive passes differ, a new view with
    the same seed repeats both, first_pass = 1 starts at the second, another seed gives another table;
    each against the reference's table for that pass."""
    loader = _loader()

    def passes(view, k):
        out = []
        for _ in range(k):
            rows, batches = [], []
            for a, p in view:
                rows.append(view.last_params.clone())
                batches.append((a, p))
            out.append((torch.cat(rows), torch.cat([a for a, _ in batches]), torch.cat([p for _, p in batches])))
        return out

    first = passes(_pairs(loader, 'norm', augment=_augment('all'), copy=True), 2)
    assert not torch.equal(first[0][0], first[1][0]) and not torch.equal(first[0][2], first[1][2])
    for k in range(2):
        assert _bits(_np(first[k][0]), _reference('all', 'norm', k)[0])
        assert _bits(_np(first[k][2]), _reference('all', 'norm', k)[2])
    again = passes(_pairs(loader, 'norm', augment=_augment('all'), copy=True), 2)
    assert all(torch.equal(x, y) for k in range(2) for x, y in zip(first[k], again[k]))
    later = passes(_pairs(loader, 'norm', augment=_augment('all', first_pass=1), copy=True), 1)
    assert all(torch.equal(x, y) for x, y in zip(later[0], first[1]))
    from a2m.data import Augment
    other = passes(_pairs(loader, 'norm', augment=Augment(seed=_seed() + 1, **SETTINGS['all']), copy=True), 1)
    assert not torch.equal(other[0][0], first[0][0])


def test_buffers_are_reused_unless_copy():
    loader = _loader()
    view = _pairs(loader, 'norm', augment=_augment('all'))
    kept = [(a.data_ptr(), p.data_ptr(), view.last_params.data_ptr()) for a, p in view]
    assert kept[0] == kept[1] != kept[2]
    params, audio, pose = _reference('all', 'norm')
    assert _bits(_np(view.last_params), params[10:])         # the 3-clip buffers hold the last batch
    styled = list(_pairs(loader, 'norm', augment=_augment('all'), copy=True, with_style=True))
    assert [len(b) for b in styled] == [3, 3, 3] and styled[0][2].dtype == torch.int32
    assert _bits(_np(styled[1][1]), pose[5:10]) and _bits(_np(styled[1][0]), audio[5:10])


# ------------------------------------------------------------------------------ data-parallel slices
def test_two_ranks_partition_the_single_device_augmented_batches():
    """Ranks 0 and 1 of world 2 and a world-1 loader, generators seeded alike, shuffled, two passes:
    per global batch of n clips the ranks' batches concatenated are its first 2 (n // 2) rows -- the
    parameters depend on the clip's table position, not on the rank or the batch."""
    def gen():
        return torch.Generator().manual_seed(3)

    whole = _loader(shuffle=True, generator=gen(), batch_size=4)
    ranks = [_loader(shuffle=True, generator=gen(), batch_size=4, rank=r, world=2) for r in range(2)]
    views = [_pairs(ld, 'norm', augment=_augment('all'), copy=True) for ld in [whole] + ranks]
    for _ in range(2):
        full, part0, part1 = (list(v) for v in views)
        assert len(full) == 4 and len(part0) == len(part1) == 3
        for k in range(3):
            for j in range(2):
                assert part0[k][j].shape[0] == 2
                assert torch.equal(torch.cat([part0[k][j], part1[k][j]]), full[k][j]), (k, j)


# ------------------------------------------------------------------------------ capture and synchronisation
def test_both_launches_capture_and_follow_order_and_pass():
    """The draw and the augmenting gather of 4 clips recorded in one graph: the replay equals the eager
    pair, and after the device order and the pass scalar are overwritten the same graph gives the new
    permutation's batch for the new pass."""
    from a2m.data import MODE_NECKSUB, MODE_STANDARDISE
    loader = _loader()
    aug = _augment('all')
    pm, ps, am, asd = _dev(PM, PS, AM, ASD)
    specs = [(P.AUDIO, MODE_STANDARDISE, am, asd), (P.POSE, MODE_NECKSUB, pm, ps)]
    g = np.random.default_rng(3)
    perm1, perm2 = g.permutation(N), g.permutation(N)

    def eager(perm, pass_):
        order_dev = loader.upload('train', perm)
        pass_dev = torch.tensor([pass_], dtype=torch.int64).to(DEV)
        params = aug.draw(order_dev, 4, 4, pass_dev, 128, T)
        return [params] + loader.gather_augmented(order_dev, 4, 4, specs, params, mask_fill=aug.mask_fill)

    eager1, eager2 = eager(perm1, 0), eager(perm2, 5)
    assert _bits(_np(eager2[0]), _draw('all', perm2[4:8], 5, _seed()))
    assert not torch.equal(eager1[0], eager2[0]) and not torch.equal(eager1[2], eager2[2])
    order_dev = loader.upload('train', perm1)
    pass_dev = torch.zeros(1, dtype=torch.int64, device=DEV)
    params = torch.zeros(4, 8, device=DEV)
    outs = [torch.zeros_like(t) for t in eager1[1:]]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        aug.draw(order_dev, 4, 4, pass_dev, 128, T, params)
        loader.gather_augmented(order_dev, 4, 4, specs, params, outs, aug.mask_fill)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip([params] + outs, eager1))
    order_dev.copy_(loader.upload('train', perm2))
    pass_dev.fill_(5)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip([params] + outs, eager2))


def test_augmented_pass_does_not_synchronise():
    """After iter() has uploaded the order and the pass number, the whole augmented pass runs under
    torch's sync debug mode 'error', as test_gpu_data.py checks the plain pass."""
    loader = _loader()
    view = _pairs(loader, 'norm', augment=_augment('all'))
    assert sum(1 for _ in view) == 3                        # buffers and both code objects exist from here on
    it = iter(view)                                         # pass 1: the uploads
    torch.cuda.synchronize()
    probe = torch.ones(1, device=DEV)
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode('error')
    try:
        try:
            probe.item()
            honoured = False
        except RuntimeError:
            honoured = True
        if honoured:
            seen = [(a, p) for a, p in it]
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    if not honoured:
        pytest.skip("the installed ROCm torch does not honour torch.cuda.set_sync_debug_mode('error')")
    assert [a.shape[0] for a, _ in seen] == [5, 5, 3]
    params, audio, pose = _reference('all', 'norm', 1)
    assert _bits(_np(seen[1][1]), pose[5:10]) and _bits(_np(seen[2][0]), audio[10:])
    assert _bits(_np(view.last_params), params[10:])


# ------------------------------------------------------------------------------ fit
def _fit_loader():
    from a2m import normalization as NZ
    loader = _loader(0, arrays={i: ARR[i] for i in 'AC'}, table=_table(('train', 'dev'), ['A', 'C']), batch_size=2)
    assert len(loader.train) == 1 and len(loader.dev) == 1
    return (loader, *NZ.get_mean_std_necksub(loader))


QUIET = dict(log_every=1, log=lambda s: None)


def test_fit_with_the_default_augment_records_the_same_losses():
    """A in train, C in dev, one batch each (test_gpu_data's fit case): one epoch on
    pairs(augment=Augment()) records exactly what one epoch on pairs() records, with identically
    initialised trainers -- the same launches on the same values."""
    from a2m.data import Augment
    loader, m, s = _fit_loader()
    want = _trainer().fit(loader.pairs('train', m, s), loader.pairs('dev', m, s), 1, **QUIET)
    got = _trainer().fit(loader.pairs('train', m, s, augment=Augment(seed=4)), loader.pairs('dev', m, s), 1, **QUIET)
    assert len(got['train_g']) == 1 and len(got['val_terms']) == 1
    assert got == want


def test_fit_with_augmentation_leaves_the_dev_pass_alone():
    """A non-trivial Augment on the train view: fit runs, its records are finite and differ from the
    unaugmented run's, and the dev batch -- formed last, in the buffers the train batch used -- is
    the unaugmented one."""
    from a2m.data import Augment
    loader, m, s = _fit_loader()
    dev = list(loader.pairs('dev', m, s, copy=True))
    train = list(loader.pairs('train', m, s, copy=True))
    aug = Augment(seed=4, p_mirror=1., speed=0.3, scale=0.2, gain=1., freq_mask=20, time_mask=8)
    view = loader.pairs('train', m, s, augment=aug)
    got = _trainer().fit(view, loader.pairs('dev', m, s), 1, **QUIET)
    assert view.passes == 1 and view.last_params[0, 0].item() == 1
    assert all(np.isfinite(v) for v in got['val_terms'][0].values()) and np.isfinite(got['train_g'][0])
    assert all(torch.equal(x, y) for x, y in zip(loader._buffers[1], dev[0]))
    augmented = list(loader.pairs('train', m, s, augment=aug, copy=True))
    assert not torch.equal(augmented[0][1], train[0][1]) and not torch.equal(augmented[0][0], train[0][0])
    assert all(torch.equal(x, y) for x, y in zip(list(loader.pairs('dev', m, s, copy=True))[0], dev[0]))
