"""a2m.data.PatsLoader on the device against the reference loader's slicing restated in numpy
(tests/pats_data_ref.py): raw batches, the batch dict's idx / style / meta, the standardise and
neck-sub modes of a2m_batch_gather_f32 bit for bit, the statistics helpers, graph capture, a pass
without host synchronisation, the data-parallel slices and GANTrainer.fit.

Bitwise equality is demanded wherever the kernel copies or applies correctly rounded float32
subtractions and divisions in a fixed order (numpy float32 arithmetic is the same three roundings).
The shapes are those of pats_data_ref: N = 13 clips in batches of 4, 4, 4, 1 at hop 5."""
import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader

import pats_data_ref as P
from test_gpu_validate import _parity, _trainer

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
ARR = P.arrays()
IDS = list('ABCD')
# A, B speak as 'oliver', C, D as 'seth'; the speaker list puts seth first: styles 1, 1, 0, 0
SPEAKERS = ['seth', 'oliver']
STYLE = {'A': 1.0, 'B': 1.0, 'C': 0.0, 'D': 0.0}


def _table(datasets=('train',) * 4, ids=IDS):
    return [P.row(d, i, 'oliver' if i in 'AB' else 'seth') for d, i in zip(datasets, ids)]


def _loader(hop=5, shuffle=False, **kw):
    from a2m.data import PatsLoader
    kw.setdefault('table', _table())
    kw.setdefault('batch_size', 4)
    return PatsLoader(kw.pop('arrays', ARR), speaker=SPEAKERS, time=P.TIME, fs_new=P.FS_NEW, window_hop=hop,
                      shuffle=shuffle, device=DEV, **kw)


def _np(t):
    return t.detach().cpu().numpy()


def _stats(seed=11):
    """Pose mean / std with std[0] = std[52] = 1 as get_mean_std_necksub gives them; audio mean / std
    with one std entry below the 1e-7 guard."""
    g = np.random.default_rng(seed)
    pm = (g.standard_normal(104) * 30).astype(np.float32)
    ps = (g.random(104) * 50 + 5).astype(np.float32)
    pm[[0, 52]], ps[[0, 52]] = 0.0, 1.0
    am = (g.standard_normal(128) - 4).astype(np.float32)
    asd = (g.random(128) * 2 + 0.5).astype(np.float32)
    asd[5] = 1e-8
    return pm, ps, am, asd


def _dev(*a):
    return [torch.from_numpy(x).to(DEV) for x in a]


def _torch_order(n, seed, passes=1):
    torch.manual_seed(seed)
    return [np.concatenate([b.numpy() for b in DataLoader(range(n), batch_size=4, shuffle=True)]) for _ in range(passes)]


# ------------------------------------------------------------------------------ raw batches and the dict
@pytest.mark.parametrize('hop', [5, 0])
@pytest.mark.parametrize('shuffle', [False, True], ids=['arange', 'seed0'])
def test_train_batches_are_the_reference_slices(hop, shuffle):
    """Every batch of .train: both modalities bitwise data[start:end:interval] stacked in idx order,
    idx the global index, style the speaker position over T frames, meta as MiniData's (interval id,
    start and end seconds, local index), start / end also against PatsClip.meta of the owning interval."""
    from a2m.windowing import PatsClip
    smp = P.samples(IDS, hop)
    n = len(smp)
    assert n == sum(P.COUNTS[hop])
    loader = _loader(hop, shuffle)
    order = _torch_order(n, 0)[0] if shuffle else np.arange(n)
    if shuffle:
        torch.manual_seed(0)
    batches = list(loader.train)
    assert len(batches) == len(loader.train) == -(-n // 4)
    clips = {i: PatsClip(ARR[i], P.FS_NEW, P.TIME, hop) for i in IDS}         # index arithmetic only: host arrays
    for k, batch in enumerate(batches):
        idx = order[4 * k:4 * k + 4]
        assert sorted(batch) == sorted([P.POSE, P.AUDIO, 'idx', 'style', 'meta'])
        assert batch['idx'].dtype == torch.int64 and np.array_equal(_np(batch['idx']), idx)
        for mod, C in ((P.POSE, 104), (P.AUDIO, 128)):
            got = batch[mod]
            assert got.is_cuda and got.dtype == torch.float32 and got.shape == (len(idx), 64, C)
            assert np.array_equal(_np(got), P.stack(ARR, smp, idx, mod, hop)), (k, mod)
        want_style = np.array([[STYLE[smp[i][0]]] * 64 for i in idx], np.float32)
        assert batch['style'].dtype == torch.float32 and np.array_equal(_np(batch['style']), want_style)
        meta = batch['meta']
        assert meta['interval_id'] == [smp[i][0] for i in idx]
        assert meta['idx'].tolist() == [smp[i][1] for i in idx]
        for j, i in enumerate(idx):
            iid, local = smp[i]
            a_start = P.starts(P.LENGTHS[iid][1], P.AUDIO, hop)[local]
            start = len(range(0, a_start, 6)) / 15
            assert meta['start'][j].item() == start and meta['end'][j].item() == start + 64 / 15
            assert [meta['start'][j].item(), meta['end'][j].item()] == clips[iid].meta([local])[0].tolist()
    if hop == 5:
        assert [len(b['idx']) for b in batches] == [4, 4, 4, 1]
        assert {smp[i][0] for i in order[:13]} == {'A', 'C', 'D'}
    again = list(loader.train)                                             # re-iterable; a new draw when shuffled
    assert len(again) == len(batches)
    if shuffle and hop == 5:
        second = _torch_order(n, 0, passes=2)[1]
        assert not np.array_equal(second, order)
        assert np.array_equal(np.concatenate([_np(b['idx']) for b in again]), second)


def test_update_dataloaders_switches_the_hop():
    loader = _loader(5)
    loader.update_dataloaders(P.TIME, 0)
    smp = P.samples(IDS, 0)
    (batch,) = list(loader.train)
    assert _np(batch['idx']).tolist() == [0, 1, 2] and batch['meta']['interval_id'] == ['A', 'C', 'D']
    for mod in (P.POSE, P.AUDIO):
        assert np.array_equal(_np(batch[mod]), P.stack(ARR, smp, [0, 1, 2], mod, 0))


def test_arrays_round_trip_through_npz(tmp_path):
    from a2m.data import PatsLoader
    path = str(tmp_path / 'arrays.npz')
    PatsLoader.save_arrays(path, ARR)
    loader = _loader(5, arrays=path)
    smp = P.samples(IDS, 5)
    last = list(loader.train)[-1]
    assert np.array_equal(_np(last[P.AUDIO]), P.stack(ARR, smp, [12], P.AUDIO, 5))


# ------------------------------------------------------------------------------ pairs: the three modes
def test_pairs_normalise_bitwise():
    """Mode 2 on the poses (subtract neck, subtract mean, divide by std) and mode 1 on the audio
    ((x - mean) / (std < 1e-7 ? 1 : std), one std entry below the guard), every batch bit for bit, the
    last batch of one clip (b0 = 12) included; without statistics both are raw."""
    smp = P.samples(IDS, 5)
    pm, ps, am, asd = _stats()
    loader = _loader(5)
    got = list(loader.pairs('train', *_dev(pm, ps, am, asd), copy=True))
    raw = list(loader.pairs('train', copy=True))
    mixed = list(loader.pairs('train', *_dev(pm, ps), copy=True))
    assert [a.shape[0] for a, _ in got] == [4, 4, 4, 1]
    for k in range(4):
        idx = np.arange(13)[4 * k:4 * k + 4]
        pose, audio = P.stack(ARR, smp, idx, P.POSE, 5), P.stack(ARR, smp, idx, P.AUDIO, 5)
        assert got[k][0].shape == (len(idx), 64, 128) and got[k][1].shape == (len(idx), 64, 104)
        assert np.array_equal(_np(got[k][1]), P.necksub_normalise(pose, pm, ps)), k
        assert np.array_equal(_np(got[k][0]), P.standardise(audio, am, asd)), k
        assert np.array_equal(_np(got[k][0])[..., 5], audio[..., 5] - am[5])          # the guarded column
        assert not _np(got[k][1])[..., [0, 52]].any()                                  # the neck itself: (0 - 0) / 1
        assert np.array_equal(_np(raw[k][0]), audio) and np.array_equal(_np(raw[k][1]), pose)
        assert np.array_equal(_np(mixed[k][0]), audio) and torch.equal(mixed[k][1], got[k][1])
    with pytest.raises(ValueError, match='come together'):
        loader.pairs('train', pose_mean=_dev(pm)[0])


def test_pairs_reuse_their_buffers_unless_copy():
    loader = _loader(5)
    pm, ps, am, asd = _dev(*_stats())
    kept = [(a.data_ptr(), p.data_ptr()) for a, p in loader.pairs('train', pm, ps, am, asd)]
    assert kept[0] == kept[1] == kept[2] != kept[3]
    fresh = list(loader.pairs('train', pm, ps, am, asd, copy=True))
    assert len({a.data_ptr() for a, _ in fresh}) == 4


def test_pairs_of_one_interval_equal_patsclip_and_necksub_normalize():
    from a2m.normalization import necksub_normalize
    from a2m.windowing import PatsClip
    pm, ps, _, _ = _dev(*_stats())
    loader = _loader(5, arrays={'D': ARR['D']}, table=_table(('train',), ['D']), batch_size=8)
    ((audio, pose),) = list(loader.pairs('train', pm, ps))
    clip = PatsClip({m: torch.from_numpy(ARR['D'][m]).to(DEV) for m in (P.POSE, P.AUDIO)}, P.FS_NEW, P.TIME, 5)
    assert len(clip) == 8
    ref = clip.batch(np.arange(8))
    assert torch.equal(audio, ref[P.AUDIO])
    assert torch.equal(pose, necksub_normalize(ref[P.POSE], pm, ps))


def test_caller_order_reversed_and_out_of_range():
    smp = P.samples(IDS, 5)
    pm, ps, am, asd = _stats()
    loader = _loader(5)
    rev = np.arange(13)[::-1].copy()
    got = list(loader.pairs('train', *_dev(pm, ps, am, asd), copy=True, order=rev))
    assert [a.shape[0] for a, _ in got] == [4, 4, 4, 1]
    for k in range(4):
        idx = rev[4 * k:4 * k + 4]
        assert np.array_equal(_np(got[k][1]), P.necksub_normalise(P.stack(ARR, smp, idx, P.POSE, 5), pm, ps))
        assert np.array_equal(_np(got[k][0]), P.standardise(P.stack(ARR, smp, idx, P.AUDIO, 5), am, asd))
    short = list(loader.pairs('train', copy=True, order=torch.tensor([12, 4, 4])))
    assert np.array_equal(_np(short[0][1]), P.stack(ARR, smp, [12, 4, 4], P.POSE, 5))
    for bad in ([0, 13], [-1, 2]):
        with pytest.raises(ValueError, match='outside'):
            loader.pairs('train', order=bad)
    with pytest.raises(ValueError, match='outside'):
        loader.pairs('dev', order=[0])


# ------------------------------------------------------------------------------ the statistics helpers
def test_mean_std_helpers_run_on_the_loader():
    """get_mean_std_necksub / get_mean_std over loader.train against float64 numpy on the same
    batches (per-batch means averaged equally, std = sqrt(E[x^2] - mean^2), std[0] = std[52] = 1 for the
    neck-subtracted variant), within 1e-5 of the largest entry as tests/test_gpu_eval.py bounds them."""
    from a2m import normalization as NZ
    smp = P.samples(IDS, 5)
    loader = _loader(5)
    batches = [P.stack(ARR, smp, np.arange(13)[k:k + 4], P.POSE, 5) for k in range(0, 13, 4)]
    for fn, sub in ((NZ.get_mean_std_necksub, True), (NZ.get_mean_std, False)):
        mean, std = fn(loader)
        xs = [(P.necksub(b) if sub else b).astype(np.float64).reshape(-1, 104) for b in batches]
        rm = np.mean([x.mean(0) for x in xs], 0)
        rs = np.sqrt(np.mean([(x * x).mean(0) for x in xs], 0) - rm * rm)
        if sub:
            rs[[0, 52]] = 1.0
        e_m, e_s = np.abs(_np(mean) - rm).max() / np.abs(rm).max(), np.abs(_np(std) - rs).max() / np.abs(rs).max()
        print(f'DATA moments necksub={sub}: mean err {e_m:.3e}, std err {e_s:.3e}')
        assert e_m <= 1e-5 and e_s <= 1e-5


# ------------------------------------------------------------------------------ capture and synchronisation
def test_gather_captures_and_follows_the_order():
    """One gather of 4 clips (a single kernel node) recorded in torch.cuda.graph: the replay equals the
    eager launch, and after the device order is overwritten with another permutation the same graph
    gives that permutation's batch."""
    from a2m.data import MODE_NECKSUB, MODE_STANDARDISE
    loader = _loader(5)
    pm, ps, am, asd = _dev(*_stats())
    specs = [(P.AUDIO, MODE_STANDARDISE, am, asd), (P.POSE, MODE_NECKSUB, pm, ps)]
    perm1, perm2 = _torch_order(13, 3, passes=2)
    order_dev = loader.upload('train', perm1)
    eager1 = loader.gather(order_dev, 4, 4, specs)
    eager2 = loader.gather(loader.upload('train', perm2), 4, 4, specs)
    assert not torch.equal(eager1[1], eager2[1])
    outs = [torch.zeros_like(t) for t in eager1]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loader.gather(order_dev, 4, 4, specs, outs)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(outs, eager1))
    order_dev.copy_(loader.upload('train', perm2))
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(outs, eager2))


def test_pairs_pass_does_not_synchronise():
    """After iter() has drawn and uploaded the permutation, the whole pass runs under torch's sync debug
    mode 'error', as tests/test_gpu_validate.py checks the validation loop: no copy to the host, no
    blocking upload."""
    smp = P.samples(IDS, 5)
    pm, ps, am, asd = _stats()
    loader = _loader(5, shuffle=True)
    pairs = loader.pairs('train', *_dev(pm, ps, am, asd))
    assert sum(1 for _ in pairs) == 4                      # buffers and the kernel's code object exist from here on
    torch.manual_seed(0)
    it = iter(pairs)                                       # the draw and the one upload
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
    assert [a.shape[0] for a, _ in seen] == [4, 4, 4, 1]
    order = _torch_order(13, 0)[0]
    # the buffers of the 4-clip batches hold the third batch, the 1-clip buffers the last
    assert np.array_equal(_np(seen[2][1]), P.necksub_normalise(P.stack(ARR, smp, order[8:12], P.POSE, 5), pm, ps))
    assert np.array_equal(_np(seen[3][0]), P.standardise(P.stack(ARR, smp, order[12:], P.AUDIO, 5), am, asd))


# ------------------------------------------------------------------------------ data-parallel slices
def test_two_ranks_partition_the_single_device_batches():
    """Ranks 0 and 1 of world 2 and a world-1 loader, generators seeded alike, in one process: per
    global batch of n clips the ranks' batches concatenated are its first 2 (n // 2) rows; the last
    batch (n = 1) is skipped on both ranks and its clip counted as dropped."""
    def gen():
        return torch.Generator().manual_seed(3)

    whole = _loader(5, shuffle=True, generator=gen())
    ranks = [_loader(5, shuffle=True, generator=gen(), rank=r, world=2) for r in range(2)]
    pm, ps, am, asd = _dev(*_stats())
    for _ in range(2):                                      # two passes: the generators advance alike
        full = list(whole.train)
        parts = [list(r.train) for r in ranks]
        assert [len(p) for p in parts] == [3, 3] == [len(r.train) for r in ranks] and len(full) == 4
        for k in range(3):
            for key in (P.POSE, P.AUDIO, 'idx', 'style'):
                both = torch.cat([parts[0][k][key], parts[1][k][key]])
                assert torch.equal(both, full[k][key][:4]), (k, key)
            assert parts[0][k]['meta']['interval_id'] + parts[1][k]['meta']['interval_id'] == full[k]['meta']['interval_id']
            assert parts[0][k]['idx'].shape[0] == 2
    assert [r.dropped['train'] for r in ranks] == [1, 1] and whole.dropped['train'] == 0
    full = list(whole.pairs('train', pm, ps, am, asd, copy=True))
    parts = [list(r.pairs('train', pm, ps, am, asd, copy=True)) for r in ranks]
    for k in range(3):
        for j in range(2):
            assert torch.equal(torch.cat([parts[0][k][j], parts[1][k][j]]), full[k][j])


# ------------------------------------------------------------------------------ fit
def test_fit_on_the_loader_equals_fit_on_lists():
    """A in train, C in dev, hop 0, batch_size 2: one batch each.  fit on loader.pairs(...) (reused
    buffers: the train and the dev batch share them) against fit on the same two batches materialised
    as lists, with a second, identically initialised trainer.  The two runs issue the same launches on
    the same values, and the library has no floating-point atomics (every reduction runs in a fixed
    order), so the loss records are compared for equality, bit for bit; the parity bar of
    tests/test_gpu_validate.py (_parity, rel 1e-4) is checked first so that a miss shows its size."""
    from a2m import normalization as NZ
    loader = _loader(0, arrays={i: ARR[i] for i in 'AC'}, table=_table(('train', 'dev'), ['A', 'C']), batch_size=2)
    assert len(loader.train) == 1 and len(loader.dev) == 1 and len(loader.test) == 0
    m, s = NZ.get_mean_std_necksub(loader)
    lists = [list(loader.pairs(split, m, s, copy=True)) for split in ('train', 'dev')]
    assert lists[0][0][1].shape == (1, 64, 104) and not torch.equal(lists[0][0][1], lists[1][0][1])
    quiet = dict(log_every=1, log=lambda s: None)
    got = _trainer().fit(loader.pairs('train', m, s), loader.pairs('dev', m, s), 1, **quiet)
    want = _trainer().fit(lists[0], lists[1], 1, **quiet)
    print(f'DATA fit bitwise equal: {got == want}')
    assert len(got['train_g']) == 1 and len(got['val_terms']) == 1
    for key in ('train_g', 'train_d', 'val_g', 'val_d'):
        assert got[key] == pytest.approx(want[key], rel=1e-4), key
    _parity(got['val_terms'][0], want['val_terms'][0])
    assert got == want
    assert all(np.isfinite(v) for v in got['val_terms'][0].values())
