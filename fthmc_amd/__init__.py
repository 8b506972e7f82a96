"""fthmc_amd -- MI355X-native (gfx950) hot path of field-transformation HMC for
2D U(1) lattice gauge theory, behind the Python API of nftqcd/fthmc."""
__version__ = '0.1.0'

# the samplers beyond the reference that a caller reaches from the package itself; resolved on first use (importing the package
# loads neither PyTorch nor the library)
_LAZY = {'MetaPotential': 'meta', 'run_meta': 'meta', 'run_ft_meta': 'meta', 'run_ptbc': 'defect', 'run_ft_ptbc': 'defect'}
__all__ = sorted(_LAZY)


def __getattr__(name):
    if name in _LAZY:
        import importlib
        return getattr(importlib.import_module(f'{__name__}.{_LAZY[name]}'), name)
    raise AttributeError(f'module {__name__!r} has no attribute {name!r}')
