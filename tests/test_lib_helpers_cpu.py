"""The Python side of the C ABI's call convention (``_lib.launch``) and the buffer helpers next to it, without a device:
``launch`` against a recording stand-in for the library, then against the real library with a NULL stream on calls its
argument checks turn away before any HIP call; ``flat_views`` on the CPU."""
import ctypes

import pytest
import torch

from eventclip_amd import _lib


class _Fake:
    """Stands in for the loaded library: ``ec_fake`` records what it is called with and returns ``rc``."""

    def __init__(self, rc=0):
        self.rc, self.got = rc, None

    def ec_fake(self, *args):
        self.got = args
        return self.rc

    def ec_last_error(self):
        return b'the fake said no'


def test_launch_converts_arguments_and_appends_the_stream(monkeypatch):
    fake, stream = _Fake(), object()
    monkeypatch.setattr(_lib, '_lib', fake)
    monkeypatch.setattr(_lib, 'stream_ptr', lambda: stream)
    t = torch.arange(4.)
    prm = _lib.EcGemmArgs()
    ref = ctypes.byref(prm)
    _lib.launch('ec_fake', t, None, prm, 3, 0.5, ref, 12345)
    got = fake.got
    assert len(got) == 8 and got[7] is stream                      # the stream goes last
    assert type(got[0]) is int and got[0] == t.data_ptr()          # a tensor: its pointer
    assert got[1] is None                                          # None stays NULL
    assert ctypes.cast(got[2], ctypes.c_void_p).value == ctypes.addressof(prm)      # a Structure: by reference
    assert got[3] == 3 and type(got[3]) is int and got[4] == 0.5 and type(got[4]) is float
    assert got[5] is ref and got[6] == 12345                       # a byref, a host address: as they are


def test_launch_raises_under_the_entry_s_name(monkeypatch):
    monkeypatch.setattr(_lib, '_lib', _Fake(rc=_lib.EC_ERR_INVALID))
    monkeypatch.setattr(_lib, 'stream_ptr', lambda: None)
    with pytest.raises(RuntimeError, match=r'ec_fake failed \(-1\): the fake said no'):
        _lib.launch('ec_fake', 1)


def test_launch_reaches_the_library_s_argument_checks(monkeypatch):
    """The real library, NULL stream: both calls are refused by the entry's own validation, before any HIP call."""
    monkeypatch.setattr(_lib, 'stream_ptr', lambda: None)
    with pytest.raises(RuntimeError, match='ec_gemm: args is null'):
        _lib.launch('ec_gemm', None)
    t = torch.zeros(4)
    with pytest.raises(RuntimeError, match=r'ec_adam_step: n=4 step=0'):
        _lib.launch('ec_adam_step', t, t, t, t, 4, .1, .9, .99, 1e-8, 0., 0)


def test_flat_views_lays_the_names_out_in_mapping_order():
    shapes = {'b': (2, 3), 'a': (), 'c': torch.Size([5])}
    flat, views = _lib.flat_views(shapes, 'cpu')
    assert flat.dtype == torch.float32 and flat.numel() == 12 and not flat.any()
    assert list(views) == ['b', 'a', 'c']
    assert [(v.storage_offset(), tuple(v.shape)) for v in views.values()] == [(0, (2, 3)), (6, ()), (7, (5,))]
    for i, v in enumerate(views.values()):                         # the views alias the flat buffer
        v.fill_(i + 1)
    assert flat.tolist() == [1.] * 6 + [2.] + [3.] * 5
    flat.zero_()
    assert not any(bool(v.any()) for v in views.values())


def test_flat_views_honours_min_numel():
    flat, views = _lib.flat_views({}, 'cpu', min_numel=4)
    assert flat.numel() == 4 and views == {}
    flat, views = _lib.flat_views({'w': (3,)}, 'cpu', min_numel=4)
    assert flat.numel() == 4 and views['w'].numel() == 3
    assert _lib.flat_views({'w': (3, 2)}, 'cpu', min_numel=4)[0].numel() == 6
