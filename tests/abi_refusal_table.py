"""What the refusal tables of the C front share (tests/test_abi_refusals.py: node / cell entry points; tests/test_abi_refusals_spmm.py: the
spatial aggregation): addresses that are never dereferenced, the case list and the call that applies ONE fault to a valid argument set."""
import ctypes
import itertools

import pytest

OK, EINVAL, EALIGN, ELIMIT, EUNSUPPORTED = 0, -1, -2, -3, -4

_BUF = ctypes.create_string_buffer(1 << 16)
_BASE = (ctypes.addressof(_BUF) + 15) & ~15
_next = itertools.count()


def P():
    """A distinct 16-byte aligned, non-null address (never dereferenced)."""
    return _BASE + 16 * (next(_next) % 4000)


def PP(n):
    return [P() for _ in range(n)]


MIS = _BASE + 4         # misaligned: refused before it is read
ODD = _BASE + 2         # not even a whole float


def with_null(ptrs, i, value=None):
    out = list(ptrs)
    out[i] = value
    return out


def case_into(cases):
    """``case(fn, fault, code, *needles)`` appending to ``cases``: the call of ``fn`` with ``fault`` applied returns ``code`` and its
    message holds every needle."""
    def case(fn, fault, code, *needles):
        cases.append(pytest.param(fn, fault, code, needles, id=f'{fn}-{len(cases)}'))
    return case


def call(lib, good, fn, fault):
    """``fn`` on its valid arguments ``good[fn]`` with ``fault`` applied; a list is passed as an array of pointers."""
    args = dict(good[fn])
    assert set(fault) <= set(args), f'{fn}: unknown argument in {sorted(fault)}'
    args.update(fault)
    keep, argv = [], []
    for value in args.values():
        if isinstance(value, list):
            value = (ctypes.c_void_p * len(value))(*value)
            keep.append(value)
        argv.append(value)
    return getattr(lib, fn)(*argv)


def check_refusal(lib, good, fn, fault, code, needles, heads=None):
    """``heads``: what the message may start with (default: the entry point's name and a colon)."""
    rc = call(lib, good, fn, fault)
    message = lib.stc_last_error().decode()
    assert rc == code, f'{fn}({fault}) returned {rc}: {message}'
    if code == OK:
        return
    assert message.startswith(heads or fn + ':'), message
    for needle in needles:
        assert needle in message, f'{fn}({fault}): {needle!r} not in {message!r}'
