"""CPU: the reader that computes the ctypes binding from include/asr_hip.h (asr_study_amd/_abi.py),
on header text written here: every form it has a rule for gives exactly the expected types, and
anything it has no rule for is refused with the text quoted -- never skipped.  The real header is
judged by the compiler and by an independent scan in test_capi_host.py."""
import ctypes as C

import pytest

from asr_study_amd import _abi

HEADER = '''/* a comment; with (every { kind of
 * bracket [ and a ; in it */
#ifndef TOY_H
#define TOY_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* toy_stream_t; /* a handle; */

enum toy_status {
  TOY_OK = 0,
  TOY_ERR_INVALID = -1, /* bad (argument) */
  TOY_ERR_LAUNCH = -3
};

#define TOY_VERSION 7
#define TOY_TAPS 4
const char* toy_last_error(void);
int toy_version(void);

typedef struct toy_args {
  int M, N;               /* two on a line; */
  const float* A; int lda;
  int d, dd;
  void* planes;
  long long seg_row[16];  /* a fixed array { */
  float taps[TOY_TAPS];
  unsigned flags;
  uint32_t word; uint64_t seed; int64_t n;
  size_t bytes;
  double eps;
  const toy_stream_t* streams;
} toy_args;
typedef struct toy_window { int chunk, left, right; } toy_window;
typedef struct toy_segment {
  int64_t offset;
  float l2;
} toy_segment;
typedef void* toy_comm_t;

size_t toy_workspace_bytes(const toy_args* a, int backward);
int toy_run(const toy_args* a, const toy_window* w,
            const toy_segment* segments_dev, int n_seg,   /* spans (lines */
            double* norm_out, char* name, void* workspace,
            size_t ws_bytes, toy_stream_t stream);
int toy_scalars(unsigned u, uint32_t a, uint64_t b, int64_t c, size_t d, double e, float f,
                long long g);
int toy_comm_init(const void* id, toy_comm_t* comm_out);

#ifdef __cplusplus
}
#endif
#endif /* TOY_H */
'''


def read(text=HEADER):
    return _abi.parse(text, device_structs={'toy_segment'})


def test_every_form_gives_the_expected_types():
    abi = read()
    vp = C.c_void_p
    assert abi.structs == {
        'toy_args': [('M', C.c_int), ('N', C.c_int), ('A', vp), ('lda', C.c_int), ('d', C.c_int),
                     ('dd', C.c_int), ('planes', vp), ('seg_row', C.c_longlong * 16),
                     ('taps', C.c_float * 4), ('flags', C.c_uint), ('word', C.c_uint32),
                     ('seed', C.c_uint64), ('n', C.c_int64), ('bytes', C.c_size_t),
                     ('eps', C.c_double), ('streams', vp)],
        'toy_window': [('chunk', C.c_int), ('left', C.c_int), ('right', C.c_int)],
        'toy_segment': [('offset', C.c_int64), ('l2', C.c_float)]}
    args, window = C.POINTER(abi.classes['toy_args']), C.POINTER(abi.classes['toy_window'])
    assert abi.functions == {
        'toy_last_error': (C.c_char_p, []),
        'toy_version': (C.c_int, []),
        'toy_workspace_bytes': (C.c_size_t, [args, C.c_int]),
        # the device struct's pointer, the host double*, char* and void* are all plain addresses
        'toy_run': (C.c_int, [args, window, vp, C.c_int, vp, vp, vp, C.c_size_t, vp]),
        'toy_scalars': (C.c_int, [C.c_uint, C.c_uint32, C.c_uint64, C.c_int64, C.c_size_t,
                                  C.c_double, C.c_float, C.c_longlong]),
        'toy_comm_init': (C.c_int, [vp, vp])}
    assert abi.constants == {'TOY_VERSION': 7, 'TOY_TAPS': 4, 'TOY_OK': 0, 'TOY_ERR_INVALID': -1,
                             'TOY_ERR_LAUNCH': -3}
    assert abi.handles == ('toy_stream_t', 'toy_comm_t')
    assert abi.names == {'structs': ('toy_args', 'toy_window', 'toy_segment'),
                         'functions': ('toy_last_error', 'toy_version', 'toy_workspace_bytes',
                                       'toy_run', 'toy_scalars', 'toy_comm_init'),
                         'constants': ('TOY_VERSION', 'TOY_TAPS', 'TOY_OK', 'TOY_ERR_INVALID',
                                       'TOY_ERR_LAUNCH')}
    for name, fields in abi.structs.items():
        assert abi.classes[name]._fields_ == fields and abi.classes[name].__name__ == name
    assert C.sizeof(abi.classes['toy_window']) == 12


ANCHOR = 'int toy_version(void);'


@pytest.mark.parametrize('extra,quoted', [
    ('int toy_bad(const toy_args* a, toy_float16 x);', 'toy_float16'),               # unknown type
    ('int toy_bad(toy_args a);', 'toy_args a'),                                      # by value
    ('int toy_cb(void (*done)(int), int n);', 'void (*done)(int)'),                  # function pointer
    ('union toy_u { int i; float f; };', 'union toy_u { int i; float f; }'),         # no rule at all
    ('#define TOY_F 1.5f\ntypedef struct toy_b { int v[TOY_F]; } toy_b;', '1.5f'),   # array bound
    ('typedef struct toy_b { int v[TOY_N]; } toy_b;', 'TOY_N'),                      # unknown bound
    ('typedef struct toy_b { float *p, *q; } toy_b;', 'float *p, *q'),               # declarator
    ('typedef struct toy_b { int v; } toy_c;', 'toy_c'),                             # two names
    ('enum toy_e { TOY_A, TOY_B };', 'TOY_A'),                                       # no value
    ('#if TOY_VERSION > 3\nint toy_new(void);\n#endif', '#if TOY_VERSION > 3'),      # directive
    ('static int toy_s(void);', 'static int'),                                       # qualifier
    ('int toy_v(int n, ...);', '...'),                                               # variadic
    ('// a line comment', '// a line comment'),
    ('int toy_comm_init(void);', 'toy_comm_init is declared twice'),
    ('typedef struct toy_window { int chunk; } toy_window;', 'toy_window'),
])
def test_what_the_reader_has_no_rule_for_is_refused_and_quoted(extra, quoted):
    assert extra.split('\n')[0] not in HEADER
    with pytest.raises(_abi.HeaderError) as e:
        read(HEADER.replace(ANCHOR, ANCHOR + '\n' + extra))
    assert quoted in str(e.value), str(e.value)


def test_a_struct_pointer_is_typed_unless_the_struct_lives_on_the_device():
    typed = _abi.parse(HEADER, device_structs=())
    assert typed.functions['toy_run'][1][2] == C.POINTER(typed.classes['toy_segment'])
    assert read().functions['toy_run'][1][2] is C.c_void_p


def test_the_package_binds_what_the_reader_gives():
    """_lib.py adds Python names and nothing else; a missing header names its path."""
    from asr_study_amd import _lib
    from asr_study_amd.build import HEADER as path
    with open(path) as f:
        abi = _abi.parse(f.read())
    assert abi.functions.keys() == _lib.SIGNATURES.keys() and abi.constants == _lib.CONSTANTS
    assert _lib.ABI_VERSION == abi.constants['ASR_HIP_ABI_VERSION']
    named = {c.__name__: n for n, c in vars(_lib).items()
             if isinstance(c, type) and issubclass(c, C.Structure) and c is not C.Structure}
    assert sorted(named) == sorted(abi.structs)
    assert named['asr_relattn_args'] == 'RelAttnArgs' and named['asr_segment'] == 'Segment'
    for s, fields in abi.structs.items():
        assert getattr(_lib, named[s])._fields_ == fields
    with pytest.raises(_lib.AsrHipError) as e:
        _lib._read_abi(path + '.absent')
    assert path + '.absent' in str(e.value)
