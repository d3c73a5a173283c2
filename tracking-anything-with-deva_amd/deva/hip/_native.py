"""What the twelve bindings (`deva.hip`, `deva.hip.metrics`, `deva.hip.vos_metrics`, `deva.hip.pair_metrics`, `deva.hip.regions`,
`deva.hip.rle`, `deva.hip.mask_runs`, `deva.hip.rle_overlap`, `deva.hip.rle_text`, `deva.hip.lowres`, `deva.hip.png`, `deva.hip.jpeg`) do alike: load a library and check it against the module's `SIGNATURES` and `ABI_VERSION`, and turn a non-zero return code
into a `DevaHipError`.  Each module keeps its own `LIB_PATH` (read when `lib()` first loads, so a tool may point it elsewhere
before that), `_LIB` and texts."""
import ctypes
import os


def load(module: dict, version_symbol: str, soname: str, kernels: str) -> ctypes.CDLL:
    """the slow half of a binding's `lib()` (`module`: its globals()): load LIB_PATH, bind SIGNATURES, compare the ABI, keep it in _LIB"""
    path = module['LIB_PATH']
    if not os.path.exists(path):
        raise module['DevaHipError'](
            f'{path} not found: {kernels} are not built. Run `python __graft_entry__.py` '
            '(or `make -C tracking-anything-with-deva_amd/csrc`). There is no CPU fallback.')
    handle = ctypes.CDLL(path)
    for name, (res, args) in module['SIGNATURES'].items():
        fn = getattr(handle, name)  # AttributeError if the .so is stale
        fn.restype = res
        fn.argtypes = args
    version = getattr(handle, version_symbol)()
    if version != module['ABI_VERSION']:
        raise module['DevaHipError'](f'{soname} ABI {version} != binding {module["ABI_VERSION"]}')
    module['_LIB'] = handle
    return handle


def check(module: dict, code: int, what: str, last_error_symbol: str) -> None:
    if code != 0:
        raise module['DevaHipError'](f'{what} failed: {getattr(module["lib"](), last_error_symbol)().decode()}')
