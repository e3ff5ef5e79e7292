"""ctypes binding of libasr_hip.so (the C ABI declared in include/asr_hip.h).

This is the only place Python touches the native library.  There is NO fallback:
if the shared object is missing or fails to load, importing the product raises.

Nothing of the ABI is written here: the argument structs, SIGNATURES and CONSTANTS are computed
from the header at import (_abi.py states the type mapping), so an entry point or a field is
added in the header alone.  Only the Python names of the structs are listed below.
"""
import ctypes as C
import os

from . import _abi
from .build import HEADER

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libasr_hip.so')

c_float_p = C.POINTER(C.c_float)
c_int_p = C.POINTER(C.c_int)
c_double_p = C.POINTER(C.c_double)
void_p = C.c_void_p


class AsrHipError(RuntimeError):
    pass


def _read_abi(path):
    try:
        with open(path) as f:
            text = f.read()
    except OSError as e:
        raise AsrHipError('cannot read %s (%s): the binding of libasr_hip.so is derived from '
                          'this header' % (path, e))
    return _abi.parse(text)


_ABI = _read_abi(HEADER)
CONSTANTS = _ABI.constants      # every #define NAME <integer> and asr_status enumerator
ABI_VERSION = CONSTANTS['ASR_HIP_ABI_VERSION']
# name -> (restype, argtypes); also the list the "exports every symbol" test walks
SIGNATURES = _ABI.functions

_unnamed = dict(_ABI.classes)


def _struct(name):
    if name not in _unnamed:
        raise AsrHipError('%s declares no struct %s (or it is named twice here)' % (HEADER, name))
    return _unnamed.pop(name)


FrontendCfg = _struct('asr_frontend_cfg')
GemmArgs = _struct('asr_gemm_args')
PackArgs = _struct('asr_pack_args')
GemmHlArgs = _struct('asr_gemm_hl_args')
Conv2dArgs = _struct('asr_conv2d_args')
LstmArgs = _struct('asr_lstm_args')
LstmLnArgs = _struct('asr_lstm_ln_args')
GateGemmArgs = _struct('asr_gate_gemm_args')
RnnArgs = _struct('asr_rnn_args')
GruArgs = _struct('asr_gru_args')
GruUniArgs = _struct('asr_gru_uni_args')
LstmUniArgs = _struct('asr_lstm_uni_args')
RhnArgs = _struct('asr_rhn_args')
AttnArgs = _struct('asr_attn_args')
RelAttnArgs = _struct('asr_relattn_args')
AttnWindow = _struct('asr_attn_window')
AttnStreamArgs = _struct('asr_attn_stream_args')
AttnCrossArgs = _struct('asr_attn_cross_args')
Segment = _struct('asr_segment')
if _unnamed:
    raise AsrHipError('%s declares %s: give it a name above' % (HEADER, ', '.join(_unnamed)))

_lib = None


def load():
    """Load libasr_hip.so (once).  Raises if it is not built -- there is no
    Python/CPU fallback for the hot path."""
    global _lib
    if _lib is not None:
        return _lib
    global LIB_PATH
    LIB_PATH = os.environ.get('ASR_LIB_PATH', LIB_PATH)      # (A/B runs of two builds)
    if not os.path.exists(LIB_PATH):
        raise AsrHipError(
            'libasr_hip.so not found at %s -- build it with '
            '`python -c "import __graft_entry__ as g; g.build()"` or '
            '`python asr_study_amd/build.py`; the hot path has no CPU fallback.' % LIB_PATH)
    # torch bundles its own HIP runtime; it must be in the process before this
    # library so that both resolve to the SAME libamdhip64 (one device context).
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)     # AttributeError if the symbol is missing
        fn.restype = res
        fn.argtypes = args
    if lib.asr_version() != ABI_VERSION:
        raise AsrHipError('%s reports ABI version %d, but %s beside it, which this binding is '
                          'derived from, says ASR_HIP_ABI_VERSION %d: the library was built from '
                          'another header, rebuild it'
                          % (LIB_PATH, lib.asr_version(), HEADER, ABI_VERSION))
    _lib = lib
    return lib


def check(rc, what=''):
    if rc != 0:
        msg = load().asr_last_error()
        raise AsrHipError('%s failed (%d): %s' % (what, rc, msg.decode() if msg else ''))
