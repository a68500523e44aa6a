"""The argument checks of a2m_augment_params_f32 and a2m_batch_gather_aug_f32 (csrc/augment.hip),
which return before any launch: A2M_EINVAL with the message set for every refused case, A2M_OK for
an empty batch.  Also the ValueErrors of a2m.data.Augment and of PatsLoader.pairs(augment=), raised
on the host.  No GPU is needed: nothing is launched (the loader here keeps its tables on the CPU)."""
import ctypes

import pytest

import pats_data_ref as P


@pytest.fixture(scope='module')
def abi():
    from a2m import _native as N
    buf = (ctypes.c_float * 1024)()
    addr = (ctypes.addressof(buf) + 15) // 16 * 16          # the kernel moves float4: 16-byte aligned
    return N, addr


def _gather(N, addr, n_mod=2, C=(128, 104), window=(382, 64), interval=(6, 1), mode=(1, 2), role=(2, 1), arena=True,
            start=True, last=True, mean=(True, True), std=(True, True), out=True, order=True, params=True, perm=True,
            b0=0, n=4, arrays=True, roles=True):
    k = len(C)

    def ptrs(flags):
        flags = flags if isinstance(flags, tuple) else (flags,) * k
        return (ctypes.c_void_p * k)(*[addr if f else None for f in flags])

    def ints(v):
        return (ctypes.c_int32 * k)(*v)

    tail = (addr if order else None, b0, n, addr if params else None, addr if perm else None, 0.0, None)
    if not arrays:
        return N.lib.a2m_batch_gather_aug_f32(n_mod, *[None] * 11, *tail)
    return N.lib.a2m_batch_gather_aug_f32(n_mod, ptrs(arena), ptrs(start), ptrs(last), ints(C), ints(window),
                                          ints(interval), ints(mode), ints(role) if roles else None, ptrs(mean),
                                          ptrs(std), ptrs(out), *tail)


GATHER_REFUSED = {
    # everything a2m_batch_gather_f32 refuses
    'n_mod 0': dict(n_mod=0),
    'n_mod 5': dict(n_mod=5),
    'null arrays': dict(arrays=False),
    'null order': dict(order=False),
    'null arena': dict(arena=(True, False)),
    'null start': dict(start=(False, True)),
    'null out': dict(out=(True, False)),
    'window 0': dict(window=(0, 64)),
    'window negative': dict(window=(382, -64)),
    'interval 0': dict(interval=(6, 0)),
    'interval negative': dict(interval=(-6, 1)),
    'C not a multiple of 4': dict(C=(126, 104)),
    'mean given for raw': dict(mode=(0, 2), std=(False, True)),
    'std given for raw': dict(mode=(0, 2), mean=(False, True)),
    'mean missing for standardise': dict(mean=(False, True)),
    'std missing for standardise': dict(std=(False, True)),
    'mean missing for neck-sub': dict(mean=(True, False)),
    'std missing for neck-sub': dict(std=(True, False)),
    'neck-sub with C 128': dict(mode=(2, 2), C=(128, 104), role=(0, 1)),
    'neck-sub with C 52': dict(C=(128, 52)),
    'unknown mode': dict(mode=(1, 3), role=(2, 0)),
    'negative n': dict(n=-1),
    'negative b0': dict(b0=-4),
    # and what the augmentation adds
    'null last table': dict(last=(True, False)),
    'null last array': dict(last=False),
    'null role array': dict(roles=False),
    'null params': dict(params=False),
    'null perm': dict(perm=False),
    'unknown role 3': dict(role=(2, 3)),
    'negative role': dict(role=(-1, 1)),
    'pose role on a raw modality': dict(mode=(1, 0), mean=(True, False), std=(True, False)),
    'pose role on a standardised modality': dict(role=(1, 1)),
    'audio role on a neck-sub modality': dict(mode=(1, 2), role=(2, 2)),
}


@pytest.mark.parametrize('case', list(GATHER_REFUSED))
def test_batch_gather_aug_refuses(abi, case):
    N, addr = abi
    assert N.lib.a2m_window_gather_f32(None, 0, 0, None, 0, 0, 0, None, None, None, None) == N.A2M_EINVAL
    assert 'batch_gather_aug' not in N.last_error()
    assert _gather(N, addr, **GATHER_REFUSED[case]) == N.A2M_EINVAL, case
    assert N.last_error().startswith('batch_gather_aug:'), N.last_error()
    with pytest.raises(N.A2MError, match='batch_gather_aug'):
        N.check(N.A2M_EINVAL)


def test_batch_gather_aug_empty_batch_is_a_no_op(abi):
    N, addr = abi
    assert _gather(N, addr, n=0, arrays=False, order=False, params=False, perm=False) == 0
    assert _gather(N, addr, n=0, arena=False, start=False, last=False, out=False, mean=False, std=False,
                   order=False, params=False, perm=False) == 0
    assert _gather(N, addr, n=0, n_mod=5, arrays=False) == N.A2M_EINVAL


def _params(N, addr, order=True, b0=0, n=4, pass_=True, seed=1, p_mirror=0.5, r_speed=0.1, r_scale=0.1, r_gain=1.0,
            max_fw=20, C=128, max_tw=10, T=64, params=True):
    return N.lib.a2m_augment_params_f32(addr if order else None, b0, n, addr if pass_ else None, seed, p_mirror,
                                        r_speed, r_scale, r_gain, max_fw, C, max_tw, T, addr if params else None,
                                        None)


PARAMS_REFUSED = {
    'negative n': dict(n=-1),
    'negative b0': dict(b0=-1),
    'null order': dict(order=False),
    'null pass': dict(pass_=False),
    'null params': dict(params=False),
    'p_mirror below 0': dict(p_mirror=-0.01),
    'p_mirror above 1': dict(p_mirror=1.01),
    'p_mirror nan': dict(p_mirror=float('nan')),
    'r_speed negative': dict(r_speed=-0.1),
    'r_speed above 0.5': dict(r_speed=0.51),
    'r_speed nan': dict(r_speed=float('nan')),
    'r_scale negative': dict(r_scale=-0.1),
    'r_scale 1': dict(r_scale=1.0),
    'r_gain negative': dict(r_gain=-1.0),
    'r_gain infinite': dict(r_gain=float('inf')),
    'max_fw above C': dict(max_fw=129),
    'max_fw negative': dict(max_fw=-1),
    'max_tw above T': dict(max_tw=65),
    'max_tw negative': dict(max_tw=-1),
    'C 0': dict(C=0, max_fw=0),
    'T 0': dict(T=0, max_tw=0),
    # refused with n = 0 too: the settings are checked before the batch size
    'r_speed above 0.5, empty batch': dict(r_speed=0.75, n=0),
}


@pytest.mark.parametrize('case', list(PARAMS_REFUSED))
def test_augment_params_refuses(abi, case):
    N, addr = abi
    assert N.lib.a2m_window_gather_f32(None, 0, 0, None, 0, 0, 0, None, None, None, None) == N.A2M_EINVAL
    assert 'augment_params' not in N.last_error()
    assert _params(N, addr, **PARAMS_REFUSED[case]) == N.A2M_EINVAL, case
    assert N.last_error().startswith('augment_params:'), N.last_error()


def test_augment_params_empty_batch_is_a_no_op(abi):
    N, addr = abi
    assert _params(N, addr, n=0, order=False, pass_=False, params=False) == 0
    assert _params(N, addr, n=0, max_fw=128, max_tw=64, p_mirror=1.0, r_speed=0.5, r_scale=0.0, r_gain=0.0) == 0


# ------------------------------------------------------------------------------ the host side
BAD_SETTINGS = {
    'p_mirror above 1': dict(p_mirror=1.5),
    'p_mirror negative': dict(p_mirror=-0.1),
    'p_mirror nan': dict(p_mirror=float('nan')),
    'speed above 0.5': dict(speed=0.6),
    'speed negative': dict(speed=-0.1),
    'scale 1': dict(scale=1.0),
    'scale negative': dict(scale=-0.5),
    'gain negative': dict(gain=-1.0),
    'gain infinite': dict(gain=float('inf')),
    'freq_mask negative': dict(freq_mask=-1),
    'freq_mask fractional': dict(freq_mask=2.5),
    'time_mask negative': dict(time_mask=-3),
    'mask_fill nan': dict(mask_fill=float('nan')),
    'seed negative': dict(seed=-1),
    'seed of 65 bits': dict(seed=2 ** 64),
    'first_pass negative': dict(first_pass=-1),
}


@pytest.mark.parametrize('case', list(BAD_SETTINGS))
def test_augment_settings_are_validated(case):
    from a2m.data import Augment
    with pytest.raises(ValueError, match='Augment'):
        Augment(**BAD_SETTINGS[case])


def test_augment_defaults_and_limits_are_accepted():
    from a2m.data import Augment
    a = Augment()
    assert (a.seed, a.p_mirror, a.speed, a.scale, a.gain, a.freq_mask, a.time_mask, a.mask_fill, a.first_pass) == \
        (0, 0., 0., 0., 0., 0, 0, 0., 0)
    b = Augment(seed=2 ** 64 - 1, p_mirror=1., speed=0.5, scale=0.999, gain=10., freq_mask=128, time_mask=64,
                mask_fill=-7.5, first_pass=3)
    assert (b.seed, b.speed, b.freq_mask, b.mask_fill, b.first_pass) == (2 ** 64 - 1, 0.5, 128, -7.5, 3)


def test_pairs_refuses_what_the_augmentation_cannot_do():
    """Mirror and scale act on the neck-subtracted pose: without pose statistics they are refused;
    masks wider than the audio window (128 channels, 64 frames) are refused; tempo, gain and masks
    alone need no statistics.  Raised by pairs(), before any iteration."""
    import numpy as np
    from a2m.data import Augment, PatsLoader
    loader = PatsLoader(P.arrays(), P.table(), 'oliver', time=P.TIME, fs_new=P.FS_NEW, window_hop=5, batch_size=4,
                        device='cpu')
    pm, ps = np.zeros(104, np.float32), np.ones(104, np.float32)
    for bad in (Augment(p_mirror=0.5), Augment(scale=0.1)):
        with pytest.raises(ValueError, match='pose_mean'):
            loader.pairs('train', augment=bad)
        loader.pairs('train', pm, ps, augment=bad)
    for bad in (Augment(freq_mask=129), Augment(time_mask=65)):
        with pytest.raises(ValueError, match='exceed'):
            loader.pairs('train', pm, ps, augment=bad)
    loader.pairs('train', augment=Augment(speed=0.2, gain=1., freq_mask=128, time_mask=64))
    with pytest.raises(TypeError, match='Augment'):
        loader.pairs('train', augment={'speed': 0.2})
    with pytest.raises(ValueError, match='come together'):
        loader.pairs('train', pose_mean=pm, augment=Augment())
    assert loader.last[P.POSE].tolist()[:5] == [79] * 4 + [80 + 64 + 74]
    assert loader.last[P.AUDIO].tolist()[:5] == [479] * 4 + [480 + 382 + 399]
