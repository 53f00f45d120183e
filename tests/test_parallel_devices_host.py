"""CPU: the host side of the in-process multi-device mode of admm_hip_parlasso / admm_hip_parbp (option PAR_DEVICES) -- the
rank-to-device assignment (admm_hip_parallel_assign, no device touched), the option's forms, the options struct's ABI, and the
Python builders' handling of the option around a call."""
import ctypes

import numpy as np
import pytest


def _assign(nblocks, devices, count):
    from admm_amd._lib import parallel_assign
    return parallel_assign(nblocks, devices, count)


def test_assignment_uses_the_largest_divisor_of_the_blocks():
    assert _assign(8, "all", 8) == list(range(8))
    assert _assign(8, "all", 3) == [0, 1]                  # 3 does not divide 8: two ranks of four blocks
    assert _assign(8, "all", 1) == []                      # one rank: the single-device path
    assert _assign(6, "0,1,2,3", 4) == [0, 1, 2]
    assert _assign(6, "3,2,1,0", 4) == [3, 2, 1]           # rank r on the r-th listed device
    assert _assign(4, "0,0", 1) == [0, 0]                  # repeats: several ranks on one device (the test form)
    assert _assign(4, "1,0,1,0", 2) == [1, 0, 1, 0]
    assert _assign(3, "0,0", 1) == []                      # 2 does not divide 3


def test_assignment_off_forms():
    for v in (None, "", "0"):
        assert _assign(8, v, 8) == []


@pytest.mark.parametrize("bad", ["a", "0,,1", "-1", "0,1,", ",0", "4", "0;1", "0 ,1", "all,0"])
def test_assignment_rejects_bad_lists(bad):
    from admm_amd._lib import AdmmHipError
    with pytest.raises(AdmmHipError) as e:
        _assign(4, bad, 4)
    assert e.value.code == 1                               # ADMM_ERR_INVALID_ARG


def test_all_needs_a_device():
    from admm_amd._lib import AdmmHipError
    with pytest.raises(AdmmHipError):
        _assign(4, "all", 0)


def test_options_struct_keeps_its_size_and_par_devices_takes_reserved_0():
    from admm_amd._lib import AdmmHipOptions
    assert ctypes.sizeof(AdmmHipOptions) == 128            # 22 selectors + par_devices + reserved[9]: unchanged
    assert AdmmHipOptions.par_devices.offset == 22 * 4     # where reserved[0] was
    assert AdmmHipOptions.reserved.offset == 23 * 4


def test_par_devices_named_and_typed_forms():
    from admm_amd import _lib
    from admm_amd._lib import AdmmHipError, options
    lib = _lib.load()
    try:
        options.struct(par_devices=-1)
        assert lib.admm_hip_option_get(b"PAR_DEVICES") == b"all"
        options.struct(par_devices=3)
        assert lib.admm_hip_option_get(b"PAR_DEVICES") == b"0,1,2"
        options.struct(par_devices=0)
        assert lib.admm_hip_option_get(b"PAR_DEVICES") is None
        with pytest.raises(AdmmHipError):
            options.struct(par_devices=-2)
        with options(par_devices="0,0"):
            assert lib.admm_hip_option_get(b"ADMM_HIP_PAR_DEVICES") == b"0,0"
        assert lib.admm_hip_option_get(b"PAR_DEVICES") is None
    finally:
        options.reset()


def test_builders_restore_the_option_on_error():
    """Without a GPU the call fails (device 0 is not there): the builder's PAR_DEVICES is gone afterwards, and the thread's own
    setting is back."""
    from admm_amd import _lib, admm_bp, admm_lasso, options
    from admm_amd._lib import AdmmHipError
    lib = _lib.load()
    rng = np.random.default_rng(3)
    x = rng.standard_normal((60, 40))
    y = rng.standard_normal(60)
    try:
        options.set(PAR_DEVICES="all")
        m = admm_lasso(x, y).penalty(nlambda=3).parallel(2, devices=[0, 0])
        assert m.devices == "0,0"
        with pytest.raises(AdmmHipError):
            m.fit()
        assert lib.admm_hip_option_get(b"PAR_DEVICES") == b"all"
        xb = rng.standard_normal((20, 60))
        with pytest.raises(AdmmHipError):
            admm_bp(xb, xb[:, 0]).parallel(2, devices="0,0").fit()
        assert lib.admm_hip_option_get(b"PAR_DEVICES") == b"all"
    finally:
        options.reset()


def test_options_enter_undoes_a_partial_set():
    from admm_amd import _lib, options
    from admm_amd._lib import AdmmHipError
    lib = _lib.load()
    try:
        with pytest.raises(AdmmHipError):
            with options(**{"PAR_DEVICES": "0,0", "": "1"}):          # the empty name is refused after PAR_DEVICES was set
                pass
        assert lib.admm_hip_option_get(b"PAR_DEVICES") is None
    finally:
        options.reset()
