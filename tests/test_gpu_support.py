"""CPU: the switch guard of tests/gpu_support.py against a stub of fthmc_amd.ops that holds the three process-global switches and
records every call made to it; no library is loaded."""
import os

import pytest

import gpu_support
from gpu_support import switches

ENV = 'FTHMC_LEAP_ROWS'


class StubOps:
    def __init__(self, variant=1, small=True, dual=1):
        self.state = {'variant': variant, 'small_path': small, 'dual_path': dual}
        self.calls = []

    def __getattr__(self, name):
        verb, _, key = name.partition('_')
        if verb not in ('get', 'set') or key not in self.state:
            raise AttributeError(name)

        def call(*value):
            self.calls.append((name,) + value + ((os.environ.get(ENV),) if name == 'set_variant' else ()))
            if verb == 'get':
                return self.state[key]
            self.state[key], = value
        return call

    def written(self):
        return {c[0] for c in self.calls if c[0].startswith('set_')}


@pytest.fixture
def ops(monkeypatch):
    stub = StubOps()
    monkeypatch.setattr(gpu_support, 'ops', stub)
    return stub


def test_switches_are_put_back_after_a_normal_exit_and_after_an_exception(ops):
    found = dict(ops.state)
    with switches(variant=0, small=False, dual=3):
        assert ops.state == {'variant': 0, 'small_path': False, 'dual_path': 3}
    assert ops.state == found
    with pytest.raises(ZeroDivisionError):
        with switches(variant=0, small=False, dual=2):
            assert ops.state == {'variant': 0, 'small_path': False, 'dual_path': 2}
            1 / 0
    assert ops.state == found
    # what it found, not what the library starts with
    ops.state.update(variant=0, small_path=False, dual_path=2)
    with switches(variant=1, small=True, dual=1):
        pass
    assert ops.state == {'variant': 0, 'small_path': False, 'dual_path': 2}


def test_nested_guards_unwind_in_order(ops):
    with switches(variant=0):
        with switches(variant=1, small=False):
            with switches(small=True, dual=0):
                assert ops.state == {'variant': 1, 'small_path': True, 'dual_path': 0}
            assert ops.state == {'variant': 1, 'small_path': False, 'dual_path': 1}
        assert ops.state == {'variant': 0, 'small_path': True, 'dual_path': 1}
    assert ops.state == {'variant': 1, 'small_path': True, 'dual_path': 1}


@pytest.mark.parametrize('named,setter', [({'variant': 0}, 'set_variant'), ({'small': False}, 'set_small_path'), ({'dual': 2}, 'set_dual_path')])
def test_a_switch_that_is_not_named_is_never_written(ops, named, setter):
    with switches(**named):
        pass
    assert ops.written() == {setter}
    ops.calls.clear()
    with switches():
        pass
    assert ops.calls == []


@pytest.mark.parametrize('before', ['0', '1', None])
def test_leap_rows_restores_a_set_variable_and_deletes_an_unset_one(ops, monkeypatch, before):
    monkeypatch.delenv(ENV, raising=False)
    if before is not None:
        monkeypatch.setenv(ENV, before)
    ops.state['variant'] = 0
    with pytest.raises(ZeroDivisionError):
        with switches(leap_rows=False):
            assert os.environ[ENV] == '0'
            1 / 0
    assert os.environ.get(ENV) == before and ops.state['variant'] == 0
    # the library is made to read the variable on entry and again on exit: with the variant it has, the second time with the old
    # value or, where there was none, with the row strips on as the library starts
    reread = [c for c in ops.calls if c[0] == 'set_variant']
    assert reread == [('set_variant', 0, '0'), ('set_variant', 0, before or '1')]
    assert ops.written() == {'set_variant'}
    with switches(leap_rows=True, variant=1):
        assert os.environ[ENV] == '1' and ops.state['variant'] == 1
    assert os.environ.get(ENV) == before and ops.state['variant'] == 0


def test_the_module_fixture_holds_its_defaults_open_and_puts_back_what_it_found(ops, monkeypatch):
    monkeypatch.setattr(gpu_support.torch.cuda, 'is_available', lambda: True)
    ops.state.update(variant=0, small_path=False, dual_path=2)
    held = gpu_support.defaults_held(dual=1)
    next(held)
    assert ops.state == {'variant': 1, 'small_path': True, 'dual_path': 1}
    with pytest.raises(StopIteration):
        next(held)
    assert ops.state == {'variant': 0, 'small_path': False, 'dual_path': 2}
    monkeypatch.setattr(gpu_support.torch.cuda, 'is_available', lambda: False)
    with pytest.raises(AssertionError, match='GPU tests need an MI355X'):
        next(gpu_support.defaults_held())
    assert ops.state == {'variant': 0, 'small_path': False, 'dual_path': 2}
