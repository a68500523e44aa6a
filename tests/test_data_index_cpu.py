"""a2m.data.PatsIndex, the host-side index of the PATS loader, against torch's own ConcatDataset /
DataLoader over stub datasets of the same lengths and against restatements of dataUtils.py written
here.  No native call is made.  The shapes are those of tests/pats_data_ref.py."""
import numpy as np
import pytest
import torch
from torch.utils.data import ConcatDataset, DataLoader, Dataset

import pats_data_ref as P
from conftest import golden


class Stub(Dataset):
    """A dataset of n items that are (its tag, the local index)."""

    def __init__(self, tag, n):
        self.tag, self.n = tag, n

    def __len__(self):
        return self.n

    def __getitem__(self, k):
        if not 0 <= k < self.n:
            raise IndexError(k)
        return self.tag, k


def _index(hop=5, **kw):
    from a2m.data import PatsIndex
    kw.setdefault('table', P.table())
    kw.setdefault('speaker', ['oliver'])
    return PatsIndex(P.lengths(), time=P.TIME, fs_new=P.FS_NEW, window_hop=hop, **kw)


def _concat(hop):
    return ConcatDataset([Stub(k, n) for k, n in enumerate(P.COUNTS[hop])])


# ------------------------------------------------------------------------------ windows and the mapping
@pytest.mark.parametrize('hop', [5, 0])
def test_counts_and_index_mapping_match_concat_dataset(hop):
    ix, ref = _index(hop), _concat(hop)
    assert ix.intervals['train'] == list('ABCD')
    assert ix.sizes['train'] == P.COUNTS[hop] == [len(P.samples([i], hop)) for i in 'ABCD']
    assert ix.cumulative_sizes['train'] == ref.cumulative_sizes
    n = len(ref)
    assert ix.size('train') == n == sum(P.COUNTS[hop]) and ix.size('dev') == 0
    for idx in range(-n, n):
        assert ix.locate('train', idx) == ref[idx], idx
    with pytest.raises(ValueError, match='absolute value of index should not exceed dataset length'):
        ix.locate('train', -n - 1)
    with pytest.raises(ValueError, match='absolute value of index should not exceed dataset length'):
        ref[-n - 1]
    with pytest.raises(IndexError):
        ix.locate('train', n)
    # C: the pose alone would give 3 windows at hop 5, the audio gives 1
    if hop == 5:
        w = ix.windows['train'][2]
        assert len(w[P.POSE][0]) == 3 and len(w[P.AUDIO][0]) == 1
    for mod in (P.POSE, P.AUDIO):
        assert ix.geometry(mod) == (*P.WINDOW[mod], 64)
        for k, iid in enumerate('ABCD'):
            st, window, interval = ix.windows['train'][k][mod]
            assert st.tolist() == P.starts(P.LENGTHS[iid][mod == P.AUDIO], mod, hop)
            assert (window, interval) == P.WINDOW[mod]
            assert all(s + window <= P.LENGTHS[iid][mod == P.AUDIO] for s in st)


def test_update_dataloaders_rederives_the_tables():
    ix = _index(5)
    ix.update_dataloaders(P.TIME, 0)
    assert ix.sizes['train'] == P.COUNTS[0] and ix.cumulative_sizes['train'] == [1, 1, 2, 3]
    ix.update_dataloaders(2.0, 3)
    assert ix.geometry(P.POSE) == (30, 1, 30) and ix.geometry(P.AUDIO) == (178, 6, 30)
    assert ix.sizes['train'][1] == min(len(range(0, 64 - 30, 3)), len(range(0, 382 - 178, 18)))


@pytest.mark.parametrize('hop,case', [(5, 0), (0, 1)])
def test_window_starts_agree_with_the_reference_fixture(hop, case):
    """tests/golden/windowing.npz holds MiniData.update_idx_list's own starts and ends for a 700 /
    4200 row recording at time 4.3, fs_new (15, 15), hop 5 (case 0) and hop 0 (case 1): the same
    geometry as interval A, whose starts are therefore the fixture's below A's length - window."""
    z = golden('windowing.npz')
    lp, la, tm, h, f0, f1 = z['cases'][case]
    assert (tm, h, f0, f1) == (P.TIME, hop, *P.FS_NEW)
    ix = _index(hop)
    for mod, tag, L in ((P.POSE, 'p', P.LENGTHS['A'][0]), (P.AUDIO, 'a', P.LENGTHS['A'][1])):
        st, window, interval = ix.windows['train'][0][mod]
        ref_s, ref_e = z[f'c{case}_{tag}_starts'], z[f'c{case}_{tag}_ends']
        keep = ref_s < L - window
        assert keep.any() and np.array_equal(st, ref_s[keep]) and np.array_equal(st + window, ref_e[keep])
        assert interval == int(z[f'c{case}_{tag}_interval'])


# ------------------------------------------------------------------------------ the epoch order
@pytest.mark.parametrize('seed', [0, 1])
def test_shuffled_batches_are_the_dataloaders(seed):
    """Two passes each, under one torch.manual_seed: the idx batches are those of DataLoader(
    ConcatDataset(stubs), batch_size=4, shuffle=True), and the second pass differs from the first."""
    ix, ref = _index(5), _concat(5)
    flat = {ref[i]: i for i in range(len(ref))}

    def theirs():
        loader = DataLoader(ref, batch_size=4, shuffle=True)
        return [[flat[(int(t), int(k))] for t, k in zip(*b)] for b in loader]

    torch.manual_seed(seed)
    want = [theirs(), theirs()]
    torch.manual_seed(seed)
    got = [[b.tolist() for b in ix.batches('train', 4, True)] for _ in range(2)]
    assert got == want
    assert got[0] != got[1]
    assert [len(b) for b in got[0]] == [4, 4, 4, 1] and sorted(sum(got[0], [])) == list(range(13))
    assert all(b.dtype == np.int64 for b in ix.batches('train', 4, True))


def test_explicit_generator_is_passed_through():
    ix, ref = _index(5), _concat(5)
    g1, g2 = torch.Generator().manual_seed(5), torch.Generator().manual_seed(5)
    for _ in range(2):
        want = [b.tolist() for b in DataLoader(range(len(ref)), batch_size=4, shuffle=True, generator=g1)]
        assert [b.tolist() for b in ix.batches('train', 4, True, generator=g2)] == want
    assert torch.equal(g1.get_state(), g2.get_state())


def test_unshuffled_order_is_arange():
    ix = _index(5)
    assert np.array_equal(np.concatenate(list(ix.batches('train', 4, False))), np.arange(13))
    assert [len(b) for b in ix.batches('train', 4, False)] == [4, 4, 4, 1]
    assert list(ix.batches('dev', 4, True)) == []


# ------------------------------------------------------------------------------ tdt_split
def _rows():
    ids = ['300', '7', 'c', 'a', 'b', '12', 'z', 'y', 'x', 'w']
    sets = ['train', 'train', 'dev', 'train', 'test', 'train', 'dev', 'train', 'train', 'test']
    return [P.row(d, i, 'oliver') for d, i in zip(sets, ids)]


def _any_lengths(rows):
    return {str(r['interval_id']): {P.POSE: 100, P.AUDIO: 600} for r in rows}


def _split_index(rows, speaker=('oliver',), **kw):
    from a2m.data import PatsIndex
    return PatsIndex(_any_lengths(rows), rows, speaker if isinstance(speaker, str) else list(speaker), **kw)


def test_split_by_dataset_column():
    ix = _split_index(_rows())
    assert ix.intervals == {'train': ['12', '300', '7', 'a', 'x', 'y'], 'dev': ['c', 'z'], 'test': ['b', 'w']}
    assert all(isinstance(i, str) for ids in ix.intervals.values() for i in ids)


def test_split_by_position():
    rows = _rows()
    ix = _split_index(rows, split=(0.6, 0.2))
    ids = [r['interval_id'] for r in rows]
    n = len(ids)
    a = int(n * 0.6)
    b = int(a + n * 0.2)
    assert ix.intervals == {'train': sorted(ids[:a]), 'dev': sorted(ids[a:b]), 'test': sorted(ids[b:])}
    assert (a, b) == (6, 8)
    odd = _split_index(rows[:7], split=(0.5, 0.3))         # int(3.5) = 3, int(3 + 2.1) = 5
    assert [len(odd.intervals[s]) for s in ('train', 'dev', 'test')] == [3, 2, 2]


def test_missing_intervals_and_their_mirrored_twins():
    rows = _rows() + [P.row('train', '7|mirror', 'oliver|mirror'), P.row('train', 'a|mirror', 'oliver|mirror'),
                      P.row('train', '7|shift', 'oliver|mirror')]
    ix = _split_index(rows, speaker=['oliver', 'oliver|mirror'], missing={'7', 'y'})
    assert ix.missing == {'7', 'y', '7|mirror', 'y|mirror'}
    assert ix.intervals['train'] == sorted(['300', 'a', '12', 'x', 'a|mirror', '7|shift'])
    plain = _split_index(_rows(), missing=['7'])
    assert plain.missing == {'7'} and '7' not in plain.intervals['train']


def test_load_data_false_keeps_five():
    ix = _split_index(_rows(), load_data=False)
    assert ix.intervals == {'train': ['12', '300', '7', 'a', 'x'], 'dev': ['c', 'z'], 'test': ['b', 'w']}


def test_speakers_styles_and_the_unknown_speaker():
    rows = [P.row('train', '1', 'seth'), P.row('train', '2', 'oliver'), P.row('dev', '3', 'seth'),
            P.row('train', '4', 'jon')]
    every = _split_index(rows, speaker=['all'])
    assert every.speaker == ['seth', 'oliver', 'jon'] and every.speaker_dict == {'seth': 0, 'oliver': 1, 'jon': 2}
    assert every.style == {'1': 0, '2': 1, '3': 0, '4': 2}
    two = _split_index(rows, speaker=['jon', 'seth'])
    assert two.speaker_dict == {'jon': 0, 'seth': 1} and two.intervals['train'] == ['1', '4']
    assert two.style == {'1': 1, '3': 1, '4': 0}
    assert _split_index(rows, speaker='oliver').intervals['train'] == ['2']
    with pytest.raises(AssertionError) as e:
        _split_index(rows, speaker=['conan'])
    assert str(e.value) == "speaker `['conan']` not found"


def test_tables_are_appended_and_ids_stay_strings(tmp_path):
    """A CSV with the columns of cmu_intervals_df.csv and numeric-looking ids, then a second table
    of rows (the reference appends cmu_intervals_df_transforms.csv): ids are strings, sorted as
    strings."""
    from a2m.data import PatsIndex
    path = tmp_path / 'cmu_intervals_df.csv'
    path.write_text(P.HEADER + '\n' + 'train,1.0,2.0,100905,oliver,1.0,v.mp4,http://x\n'
                    'train,1.0,2.0,9,oliver,1.0,"v,1.mp4",http://x\n' 'dev,1.0,2.0,0012,oliver,1.0,v.mp4,http://x\n')
    more = [P.row('train', 55, 'oliver'), ('test', '1', '2', '77|m', 'oliver', '1', 'v', 'l')]
    lengths = {i: {P.POSE: 100, P.AUDIO: 600} for i in ('100905', '9', '0012', '55', '77|m')}
    ix = PatsIndex(lengths, [str(path), more], ['oliver'])
    assert ix.intervals == {'train': ['100905', '55', '9'], 'dev': ['0012'], 'test': ['77|m']}
    one = PatsIndex(lengths, path, ['oliver'])
    assert one.intervals == {'train': ['100905', '9'], 'dev': ['0012'], 'test': []}


# ------------------------------------------------------------------------------ what is not built
@pytest.mark.parametrize('name,value', [('filler', True), ('repeat_text', 0), ('style_iters', 4),
                                        ('sample_all_styles', -1), ('quantile_sample', 0.9),
                                        ('quantile_num_training_sample', 10), ('weighted', 1),
                                        ('num_training_sample', 100), ('num_training_iters', 50)])
def test_unsupported_arguments_are_named(name, value):
    from a2m.data import UNSUPPORTED
    with pytest.raises(NotImplementedError, match=name):
        _index(5, **{name: value})
    assert _index(5, **{name: UNSUPPORTED[name]}).size('train') == 13


def test_text_modalities_are_refused():
    from a2m.data import PatsIndex
    with pytest.raises(NotImplementedError, match='modalities'):
        PatsIndex(P.lengths(), P.table(), ['oliver'], modalities=(P.POSE, 'text/bert'))
    with pytest.raises(TypeError):
        _index(5, num_workers_typo=3)


# ------------------------------------------------------------------------------ data-parallel slicing
@pytest.mark.parametrize('world', [2, 3])
def test_dp_slices_partition_every_batch(world):
    """N = 13, batch_size 4: global batches of 4, 4, 4, 1.  world 2: m = 2, 2, 2, 0 (the last is
    skipped everywhere, 1 dropped); world 3: m = 1, 1, 1, 0 (1 + 1 + 1 + 1 dropped)."""
    from a2m.data import dp_plan
    ix = _index(5)
    order = ix.order('train', False)
    plans = [dp_plan(len(order), 4, r, world) for r in range(world)]
    glob = [(b0, min(4, 13 - b0)) for b0 in range(0, 13, 4)]
    live = [(b0, n) for b0, n in glob if n // world]
    assert [len(p[0]) for p in plans] == [len(live)] * world == [3] * world
    dropped = sum(n % world for _, n in glob)
    assert [p[1] for p in plans] == [dropped] * world and dropped == {2: 1, 3: 4}[world]
    for k, (g0, n) in enumerate(live):
        m = n // world
        rows = [list(range(p[0][k][0], p[0][k][0] + p[0][k][1])) for p in plans]
        assert all(len(r) == m for r in rows)
        assert sum(rows, []) == list(range(g0, g0 + m * world))          # disjoint, contiguous, in rank order
    assert dp_plan(13, 4, 0, 1) == (glob, 0)
    assert dp_plan(3, 4, 1, 4) == ([], 3) and dp_plan(0, 4, 0, 2) == ([], 0)
