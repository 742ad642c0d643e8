"""Per-sample noise streams, host side (no GPU): the three entry points are declared, bound and exported under ABI
version 2, and their argument checks refuse by name before any device work."""
import ctypes as C
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dsx_randn_samples", "dsx_sample_loop_streams", "dsx_posterior_step_streams")
ONE = 16                                                   # a non-null address that is never dereferenced


def _lib():
    from diffsplitting_amd import _lib
    return _lib


def _ids(*v):
    return (C.c_uint64 * len(v))(*v)


def _refused(rc, word):
    msg = _lib().lib.dsx_last_error()
    assert rc == -1, (rc, msg)
    assert word in msg, msg


def test_stream_symbols_declared_bound_exported():
    lib = _lib()
    header = open(os.path.join(ROOT, "include", "dsx.h")).read()
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in lib.SIGNATURES
        assert getattr(lib.lib, name) is not None
    assert lib.lib.dsx_abi_version() == 2 and re.search(r"#define\s+DSX_ABI_VERSION\s+2\b", header)
    # the definition of the streams is part of the header
    assert "(id << 24) | draw" in header
    assert (lib.STREAM_ID_LIMIT, lib.STREAM_DRAW_LIMIT) == (1 << 40, 1 << 24)


def test_existing_signatures_are_untouched():
    lib = _lib()
    assert len(lib.SIGNATURES["dsx_sample_loop"][1]) == 11
    assert len(lib.SIGNATURES["dsx_posterior_step"][1]) == 21
    assert len(lib.StepTable._fields_) == 10
    # the stream forms take the same arguments plus (ids, count)
    assert lib.SIGNATURES["dsx_sample_loop_streams"][1][:11] == lib.SIGNATURES["dsx_sample_loop"][1]
    assert lib.SIGNATURES["dsx_posterior_step_streams"][1][:21] == lib.SIGNATURES["dsx_posterior_step"][1]


def test_randn_samples_refusals():
    lib = _lib().lib
    _refused(lib.dsx_randn_samples(ONE, 2, 12, 1, None, 0, None), b"sample_ids is null")
    _refused(lib.dsx_randn_samples(ONE, 2, 12, 1, _ids(3, 1 << 40), 0, None), b"sample id")
    assert b"2^40" in lib.dsx_last_error()
    _refused(lib.dsx_randn_samples(ONE, 2, 12, 1, _ids(3, 4), 1 << 24, None), b"draw ordinal")
    _refused(lib.dsx_randn_samples(None, 2, 12, 1, _ids(3, 4), 0, None), b"randn_samples")
    _refused(lib.dsx_randn_samples(ONE, 0, 12, 1, _ids(3), 0, None), b"randn_samples")
    _refused(lib.dsx_randn_samples(ONE, 2, 0, 1, _ids(3, 4), 0, None), b"randn_samples")


def test_posterior_step_streams_refusals():
    lib = _lib().lib
    head = (ONE, ONE, 2, 1, 2, 2, ONE, ONE, ONE, ONE, ONE, 1, 0)          # x .. clip
    tail = (None, None, ONE, None)                                        # outputs, stream
    ok = _ids(5, (1 << 40) - 1)
    _refused(lib.dsx_posterior_step_streams(*head, None, 7, 1, 0, *tail, None, 2), b"sample_ids is null")
    _refused(lib.dsx_posterior_step_streams(*head, None, 7, 1, 0, *tail, ok, 3), b"sample ids for a batch of 2")
    _refused(lib.dsx_posterior_step_streams(*head, None, 7, 1, 0, *tail, _ids(5, 1 << 40), 2), b"sample id")
    _refused(lib.dsx_posterior_step_streams(*head, None, 7, 1 << 24, 0, *tail, ok, 2), b"draw ordinal")
    _refused(lib.dsx_posterior_step_streams(*head, ONE, 7, 1, 0, *tail, ok, 2), b"injected noise together with sample_ids")
    _refused(lib.dsx_posterior_step_streams(*head, None, 7, 1, 1, *tail, ok, 2), b"repeat_noise")
    _refused(lib.dsx_posterior_step_streams(*head, None, 7, 1, 0, None, None, None, None, ok, 2), b"output")


def test_sample_loop_streams_refuses_without_an_executor():
    """The executor-bound checks (id count against its batch, injected noise with ids, id and draw ranges) need an
    executor and are exercised on the device (tests/test_gpu_streams.py); without one the call is refused outright."""
    lib = _lib()
    tab = lib.StepTable()
    _refused(lib.lib.dsx_sample_loop_streams(None, C.byref(tab), None, ONE, None, 1, None, 0, None, 0, None, _ids(1), 1),
             b"null executor")


def test_python_refusals_name_the_argument():
    """engine-side checks come before the GPU is asked for."""
    from diffsplitting_amd import engine
    from diffsplitting_amd._lib import DsxError
    with pytest.raises(DsxError, match="sample id"):
        engine._sample_ids([1, 1 << 40], 2)
    with pytest.raises(DsxError, match="B = 3"):
        engine._sample_ids([1, 2], 3)
    with pytest.raises(DsxError, match="draw ordinal"):
        engine._draw_ordinal(1 << 24)
    assert engine._sample_ids([7, (1 << 40) - 1], 2).tolist() == [7, (1 << 40) - 1]


def test_sampler_keywords_exist_and_default_off():
    from diffsplitting_amd.data import tiled_predict
    from diffsplitting_amd.model import samplers as S
    for cls, names in ((S.GaussianSampler, ("p_sample_loop", "super_resolution", "predict", "sample")),
                       (S.GaussianSamplerDdpm, ("p_sample_loop", "predict")),
                       (S.InDISampler, ("inference",)), (S.JointIndiSampler, ("inference",))):
        for name in names:
            p = inspect.signature(getattr(cls, name)).parameters
            assert p["seed"].default is None and p["sample_ids"].default is None, (cls.__name__, name)
    # the single steps keep the reference's parameter lists; their stream forms are methods of their own
    for cls, name in ((S.GaussianSampler, "p_sample"), (S.GaussianSamplerDdpm, "p_sample"), (S.InDISampler, "inference_one_step")):
        assert "seed" not in inspect.signature(getattr(cls, name)).parameters
        p = inspect.signature(getattr(cls, name + "_seeded")).parameters
        assert p["seed"].default is inspect.Parameter.empty and p["sample_ids"].default is inspect.Parameter.empty
    for fn in (tiled_predict.predict_tiled, tiled_predict.predict_tiled_mixed):
        assert inspect.signature(fn).parameters["seed"].default is None


def test_sampler_refusals_without_a_device():
    from diffsplitting_amd._lib import DsxError
    from diffsplitting_amd.model import samplers as S
    s = S.InDISampler(None, 32, channels=2, conditional=False)
    assert s._draws(2, None, None).streams is None
    with pytest.raises(DsxError, match="only together with sample_ids"):
        s._draws(2, 3, None)
    with pytest.raises(DsxError, match="need seed"):
        s._draws(2, None, [1, 2])
    s.noise_source = lambda shape: None
    with pytest.raises(DsxError, match="noise_source together with sample_ids"):
        s._draws(2, 3, [1, 2])
    s.noise_source = None
    assert s._draws(2, 3, [5, 9]).streams == (3, [5, 9])
    j = S.JointIndiSampler.__new__(S.JointIndiSampler)
    assert j.second_ids([1, 2]) == [1 | 1 << 39, 2 | 1 << 39]
    with pytest.raises(DsxError, match=r"2\^39"):
        j.second_ids([1 << 39])


def test_command_lines_carry_the_flag():
    from diffsplitting_amd import infer, split
    assert "--sample-seed" in inspect.getsource(split.main) and "--sample-seed" in inspect.getsource(infer.main)
