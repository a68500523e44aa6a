"""Shared inputs and numpy restatements for the a2m.data tests (test_data_index_cpu.py,
test_gpu_data.py): four synthetic intervals, their table, and the reference loader's slicing and
normalisation written out in numpy.

(pose length, audio length) = A (80, 480), B (64, 382), C (75, 400), D (100, 600) at time 4.3,
fs_new (15, 15): pose windows are 64 rows at interval 1, log_mel_512 windows 382 rows at interval
6 (64 rows out).  With window_hop 5 the intervals hold 4, 0, 1 and 8 samples -- B is exactly one
window long and range(0, L - window) is empty; in C the audio allows 1 and the pose 3 -- so N = 13
and batch_size 4 gives batches of 4, 4, 4, 1.  With window_hop 0: 1, 0, 1, 1.  The smallest shapes
with an empty interval inside the concatenation, a minimum over modalities that decides, a last
batch of one clip and arena offsets (80, 144, 219 pose rows; 480, 862, 1262 audio rows) that are
multiples of nothing convenient."""
import numpy as np

POSE, AUDIO = 'pose/data', 'audio/log_mel_512'
LENGTHS = {'A': (80, 480), 'B': (64, 382), 'C': (75, 400), 'D': (100, 600)}
COUNTS = {5: [4, 0, 1, 8], 0: [1, 0, 1, 1]}
TIME, FS_NEW = 4.3, (15, 15)
WINDOW = {POSE: (64, 1), AUDIO: (382, 6)}       # (window, interval): int(4.3 * 15), int(4.3 * 89), round(89 / 15)
HEADER = 'dataset,delta_time,end_time,interval_id,speaker,start_time,video_fn,video_link'


def row(dataset, interval_id, speaker):
    return {'dataset': dataset, 'delta_time': '1.0', 'end_time': '2.0', 'interval_id': interval_id,
            'speaker': speaker, 'start_time': '1.0', 'video_fn': 'v.mp4', 'video_link': 'http://x'}


def table(datasets=('train', 'train', 'train', 'train')):
    return [row(d, i, 'oliver') for d, i in zip(datasets, 'ABCD')]


def lengths():
    return {i: {POSE: lp, AUDIO: la} for i, (lp, la) in LENGTHS.items()}


def arrays(seed=7):
    """Poses around 300 +- 40 (neck columns far from zero), audio around -4 +- 2."""
    g = np.random.default_rng(seed)
    return {i: {POSE: (g.standard_normal((lp, 104)) * 40 + 300).astype(np.float32),
                AUDIO: (g.standard_normal((la, 128)) * 2 - 4).astype(np.float32)}
            for i, (lp, la) in LENGTHS.items()}


def starts(length, modality, hop):
    """MiniData.update_idx_list (dataUtils.py:611-616), restated."""
    window, interval = WINDOW[modality]
    return list(range(0, length - window, window if not hop else hop * interval))


def samples(ids, hop):
    """[(interval_id, local index)] in ConcatDataset order over the intervals `ids`."""
    out = []
    for i in ids:
        n = min(len(starts(L, m, hop)) for L, m in zip(LENGTHS[i], (POSE, AUDIO)))
        out += [(i, k) for k in range(n)]
    return out


def window(arr, iid, k, modality, hop):
    """MiniData.__getitem__'s data[start:end:interval] (dataUtils.py:648-654)."""
    w, interval = WINDOW[modality]
    s = starts(LENGTHS[iid][modality == AUDIO], modality, hop)[k]
    return arr[iid][modality][s:s + w:interval]


def stack(arr, smp, idx, modality, hop):
    return np.stack([window(arr, *smp[i], modality, hop) for i in idx])


def standardise(x, mean, std):
    """(x - mean) / where(std < 1e-7, 1, std), each step one float32 rounding."""
    x, mean, std = (np.asarray(a, np.float32) for a in (x, mean, std))
    out = (x - mean) / np.where(std < np.float32(1e-7), np.float32(1), std)
    assert out.dtype == np.float32
    return out


def necksub(x):
    x = np.asarray(x, np.float32)
    out = x.copy()
    out[..., :52] -= x[..., 0:1]
    out[..., 52:] -= x[..., 52:53]
    return out


def necksub_normalise(x, mean, std):
    """((x - neck) - mean) / std: subtract neck, subtract mean, divide, each rounded to float32."""
    out = (necksub(x) - np.asarray(mean, np.float32)) / np.asarray(std, np.float32)
    assert out.dtype == np.float32
    return out
