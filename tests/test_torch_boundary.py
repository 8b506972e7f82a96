"""CPU-only tests of the torch operator boundary's two registrations (fthmc_amd/torch_ops.py): the compiled TORCH_LIBRARY
(csrc/torch_library.cpp) and the Python custom_op fallback (FTHMC_TORCH_OPS=python) define the same 20 operators with the same
schema text, the module's table is what both are made from, and every operator propagates shapes on meta tensors.  No compute
calls: there is no GPU here.  The fallback is looked at in a fresh child process (a process has one registration)."""
import json
import os
import re
import subprocess
import sys
import warnings

import pytest
import torch

from conftest import ROOT

B, L, NL = 3, 8, 2
NETS = {'default': (2, None, 3, 955), 'generic': (1, [4, 6, 5], 5, 1817)}      # n_mix, hidden, kernel_size, weights per layer
NO_FORMULA = ('wilson_loops', 'local_update', 'instanton_hit')


def _meta(*shape, dtype=torch.float64, grad=False):
    return torch.empty(*shape, dtype=dtype, device='meta', requires_grad=grad)


def _calls(n_mix, hidden, k, params, grad=False):
    """one call of every operator on meta tensors -> {name: arguments}"""
    x, v, u, bb = _meta(B, 2, L, L, grad=grad), _meta(B, 2, L, L), _meta(B), _meta(B)
    w, w_all, seeds = _meta(params), _meta(NL * params), _meta(B, dtype=torch.int64)
    net = (n_mix, hidden, k)
    K, M = 2, 2
    return {
        'wilson_action_charge': (x, 2.0), 'wilson_force': (x, 2.0), 'wilson_loops': (x, 3, 2),
        'hmc_trajectory': (x, v, u, 2.0, 0.1, 3),
        'flow_layer_fwd': (x, w, 1, 2, n_mix, 0, hidden, k),
        'flow_layer_bwd_x': (x, v, u, w, 1, 2, n_mix, 0, hidden, k),
        'flow_layer_bwd_w': (x, v, u, w, 1, 2, n_mix, 0, hidden, k),
        'flow_layer_bwd': (x, v, u, w, 1, 2, n_mix, 0, hidden, k),
        'flow_layer_rev': (x, w, 1, 2, n_mix, 0, 1e-12, hidden, k),
        'ft_action_force': (x, w_all, NL, 2.0, 0, *net),
        'fthmc_trajectory': (x, v, u, w_all, NL, 2.0, 0.1, 3, 0, 0, *net),
        'train_grad': (x, w_all, NL, 2.0, 0, *net),
        'ft_action_vjp': (x, w_all, NL, 2.0, 0, u, None, *net),
        'ft_force_vjp': (x, w_all, NL, 2.0, 0, v, *net),
        'train_force_grad': (x, w_all, NL, 2.0, 0, *net),
        'ft_trajectory_pb': (x, v, u, w_all, NL, bb, 0.1, 3, 1, 0, None, *net),
        'hmc_trajectory_pb': (x, v, u, bb, 0.1, 3, 1),
        'replica_swap': (_meta(K), _meta(M * K), _meta(M, K - 1), _meta(M * K), _meta(M * K, dtype=torch.int32),
                         _meta(M * K, dtype=torch.int32), 0),
        'local_update': (x, 2.0, bb, seeds, 1, 1),
        'instanton_hit': (x, 2.0, None, seeds, 2),
    }


def _report():
    """what this process's registration looks like, as JSON-able data (run in-process and in the FTHMC_TORCH_OPS=python child)"""
    import fthmc_amd.torch_ops as T
    O = torch.ops.fthmc_hip
    out = {'backend': T.BACKEND, 'all': list(T.__all__), 'table': [[op.name, op.schema, list(op.mutates)] for op in T.OPS],
           'schemas': {op.name: str(getattr(O, op.name).default._schema) for op in T.OPS},
           'bound': {op.name: type(getattr(T, op.name, None)).__name__ for op in T.OPS}, 'shapes': {}, 'no_formula': {}}
    for tag, net in NETS.items():
        for name, args in _calls(*net).items():
            r = getattr(T, name)(*args)
            out['shapes'][f'{tag}/{name}'] = [[list(t.shape), str(t.dtype), str(t.device)] for t in (r if isinstance(r, (tuple, list)) else (r,))]
    # keyword arguments and omitted defaults reach the shape functions too
    y, lj = O.flow_layer_fwd(_meta(B, 2, L, L), _meta(1817), 0, 1, act=0, n_mix=1, kernel_size=5, hidden=[4, 6, 5])
    out['shapes']['keywords/flow_layer_fwd'] = [list(y.shape), list(lj.shape)]
    # a backward through an operator without a formula
    for name in NO_FORMULA:
        r = getattr(O, name)(*_calls(*NETS['default'], grad=True)[name])
        r = r[0] if isinstance(r, (tuple, list)) else r
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter('always')
            try:
                r.sum().backward()
                how = 'passes'
            except RuntimeError as e:
                how = 'raises: ' + str(e)
        out['no_formula'][name] = [r.requires_grad, how, [str(w.message) for w in caught if 'autograd kernel was not registered' in str(w.message)]]
    return out


@pytest.fixture(scope='module')
def reports():
    for so in ('libfthmc_hip.so', 'libfthmc_torch.so'):
        if not os.path.exists(os.path.join(ROOT, 'fthmc_amd', so)):
            pytest.skip(f'{so} not built (make -C fthmc_amd/csrc)')
    if os.environ.get('FTHMC_TORCH_OPS', '') == 'python':
        pytest.skip('this process was asked for the Python registration: the compiled one cannot be looked at in it')
    code = ('import sys, json; sys.path[:0] = [%r, %r]; import test_torch_boundary as m; print(json.dumps(m._report()))'
            % (ROOT, os.path.join(ROOT, 'tests')))
    p = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, FTHMC_TORCH_OPS='python'), cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    child = json.loads([l for l in p.stdout.splitlines() if l.startswith('{')][-1])
    here = _report()
    assert here['backend'] == 'compiled' and child['backend'] == 'python'
    return {'compiled': here, 'python': child}


def test_both_registrations_carry_the_tables_schema_text(reports):
    import fthmc_amd.torch_ops as T
    assert len(T.OPS) == 20 and len({op.name for op in T.OPS}) == 20
    for backend, rep in reports.items():
        assert rep['table'] == [[op.name, op.schema, list(op.mutates)] for op in T.OPS], backend
        for op in T.OPS:
            assert rep['schemas'][op.name] == 'fthmc_hip::' + op.name + op.schema, (backend, op.name)
    assert reports['compiled']['schemas'] == reports['python']['schemas']
    sch = reports['python']['schemas']
    assert 'SymInt' not in ''.join(sch.values())
    assert 'Tensor(a!) beta_b, Tensor(b!) rung, Tensor(c!) chain_of' in sch['replica_swap']
    assert [op.name for op in T.OPS if op.mutates] == ['replica_swap'] and T.OPS[16].mutates == ('beta_b', 'rung', 'chain_of')


def test_the_compiled_librarys_operator_list_is_the_table():
    """the X(name, "schema") list of csrc/torch_library.cpp, read as text: the table's rows, in the table's order"""
    import fthmc_amd.torch_ops as T
    src = open(os.path.join(ROOT, 'fthmc_amd', 'csrc', 'torch_library.cpp')).read()
    rows = re.findall(r'^\s*X\((\w+), "([^"]*)"\)', src, re.M)
    assert rows == [(op.name, op.schema) for op in T.OPS]
    assert 'm.def("' not in src and 'm.impl("' not in src            # no operator named outside the list


def test_names_are_bound_under_either_backend(reports):
    import fthmc_amd.torch_ops as T
    names = [op.name for op in T.OPS]
    assert T.__all__ == names
    for backend, rep in reports.items():
        assert rep['all'] == names, backend
        kind = {'compiled': 'OpOverloadPacket', 'python': 'CustomOpDef'}[backend]
        assert rep['bound'] == {n: kind for n in names}, backend


def test_fake_shapes_of_every_operator(reports):
    f64, i32 = 'torch.float64', 'torch.int32'
    x, b = [[B, 2, L, L], f64, 'meta'], [[B], f64, 'meta']
    for tag, (n_mix, hidden, k, params) in NETS.items():
        gw1, gw = [[params], f64, 'meta'], [[NL * params], f64, 'meta']
        want = {
            'wilson_action_charge': [b, b, b], 'wilson_force': [x], 'wilson_loops': [[[B, 3, 2], f64, 'meta']],
            'hmc_trajectory': [x, b, b],
            'flow_layer_fwd': [x, b], 'flow_layer_bwd_x': [x], 'flow_layer_bwd_w': [gw1], 'flow_layer_bwd': [x, gw1], 'flow_layer_rev': [x, b],
            'ft_action_force': [b, b, x], 'fthmc_trajectory': [x, b, b, b, b], 'train_grad': [x, b, b, gw],
            'ft_action_vjp': [x, gw], 'ft_force_vjp': [x, gw], 'train_force_grad': [x, b, gw],
            'ft_trajectory_pb': [x, b, b, b, b, [[3, B], f64, 'meta']], 'hmc_trajectory_pb': [x, b, b],
            'replica_swap': [[[2, 1], f64, 'meta'], [[2, 1], f64, 'meta']],
            'local_update': [x], 'instanton_hit': [x, [[B], i32, 'meta'], [[B], i32, 'meta']],
        }
        assert len(want) == 20
        for backend, rep in reports.items():
            for name, shapes in want.items():
                assert rep['shapes'][f'{tag}/{name}'] == shapes, (backend, tag, name)
    for rep in reports.values():
        assert rep['shapes']['keywords/flow_layer_fwd'] == [[B, 2, L, L], [B]]
        assert len(rep['shapes']) == 41


def test_backward_through_an_operator_without_a_formula(reports):
    """wilson_loops, local_update and instanton_hit carry no autograd formula.  What asking for a gradient through one does is
    the registration mechanism's and differs between the two (as it did before the table): a custom_op refuses with an error;
    the compiled library's operator falls to torch's not-implemented fallback, which warns and lets the backward pass.  Each is
    pinned as it is."""
    for name in NO_FORMULA:
        req, how, warned = reports['python']['no_formula'][name]
        assert req and how.startswith('raises: ') and 'no autograd formula was registered' in how and name in how
        req, how, warned = reports['compiled']['no_formula'][name]
        assert req and how == 'passes' and len(warned) == 1 and f'fthmc_hip::{name}' in warned[0]
