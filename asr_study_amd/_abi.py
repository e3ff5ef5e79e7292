"""Reader of include/asr_hip.h: the argument structs, entry points and constants of the C ABI as
ctypes types, computed from the header text so that no layout or signature is written twice.

The header keeps to a small subset of C: `typedef struct name { ... } name;`, prototypes,
`typedef void* name;`, one enum, `#define NAME <integer>`.  parse() cuts every construct it
recognises out of the text and REFUSES whatever is left: a declaration it has no rule for raises
HeaderError with the text quoted, it is never skipped (a skipped argument would shift every later
one by a register).  Needs neither the library nor a device.

Types: a C scalar -> its ctypes scalar; a `typedef void*` handle -> c_void_p; a `const char*`
return -> c_char_p; a pointer to an argument struct -> POINTER(its class); EVERY other pointer,
struct members included -> c_void_p whatever it points to (device addresses arrive as Python ints
and None, which typed pointers refuse).  DEVICE_STRUCTS are structs that live in device arrays: a
pointer to one is an address like any other.
"""
import collections
import ctypes as C
import re

SCALARS = {'int': C.c_int, 'unsigned': C.c_uint, 'long long': C.c_longlong, 'float': C.c_float,
           'double': C.c_double, 'size_t': C.c_size_t, 'int64_t': C.c_int64,
           'uint64_t': C.c_uint64, 'uint32_t': C.c_uint32}
POINTEES = ('void', 'char')                     # types that exist behind a '*' only
DEVICE_STRUCTS = frozenset(['asr_segment'])

# structs: name -> [(field, ctype)];  functions: name -> (restype, argtypes);  constants: name ->
# int;  names: kind -> the declared names in header order;  handles: the `typedef void*` names;
# classes: struct name -> the ctypes.Structure built from its field list
Abi = collections.namedtuple('Abi', 'structs functions constants names handles classes')


class HeaderError(ValueError):
    pass


# [const] type (* | space) name[bound] {, name[bound]}
_ITEM = r'\w+(?:\s*\[\s*\w+\s*\])?'
_DECL = re.compile(r'(const\s+)?([A-Za-z_][\w ]*?)(?:\s*(\*)\s*|\s+)(%s(?:\s*,\s*%s)*)'
                   % (_ITEM, _ITEM))
_NAME_BOUND = re.compile(r'(\w+)(?:\s*\[\s*(\w+)\s*\])?')
# what surrounds the declarations, named line by line: include guard, extern "C", includes
_FRAME = [r'^#ifndef[ \t]+(\w+)[ \t]*\n#define[ \t]+\1[ \t]*$', r'^#endif\s*\Z',
          r'^#ifdef __cplusplus[ \t]*\nextern "C" \{[ \t]*\n#endif[ \t]*$',
          r'^#ifdef __cplusplus[ \t]*\n\}[ \t]*\n#endif[ \t]*$', r'^#include[ \t]+<\w+\.h>[ \t]*$']


def parse(text, device_structs=DEVICE_STRUCTS):
    structs, classes, functions, constants, handles = {}, {}, {}, {}, []

    def integer(tok, where):
        if re.fullmatch(r'-?\d+', tok):
            return int(tok)
        if tok in constants:
            return constants[tok]
        raise HeaderError('%r is no integer in %r' % (tok, where))

    def declare(stmt):
        """'const float* A' / 'int d, dd' / 'long long row[16]' -> const, type, '*', [(name, n)]"""
        m = _DECL.fullmatch(stmt.strip())
        if not m:
            raise HeaderError('cannot parse the declarator %r' % stmt.strip())
        items = [_NAME_BOUND.fullmatch(i.strip()).groups() for i in m.group(4).split(',')]
        return bool(m.group(1)), ' '.join(m.group(2).split()), m.group(3), \
            [(n, None if b is None else integer(b, stmt.strip())) for n, b in items]

    def ctype(const, base, ptr, where, member=False, ret=False):
        if ptr:
            if (const, base, ret) == (True, 'char', True):
                return C.c_char_p
            if base in classes and base not in device_structs and not member:
                return C.POINTER(classes[base])
            if base in SCALARS or base in POINTEES or base in classes or base in handles:
                return C.c_void_p
        elif base in SCALARS:
            return SCALARS[base]
        elif base in handles:
            return C.c_void_p
        raise HeaderError('unknown type %r in %r' % (base + (ptr or ''), where.strip()))

    def one(stmt, **kw):
        """A prototype's head or parameter: exactly one name, no array."""
        const, base, ptr, items = declare(stmt)
        if len(items) != 1 or items[0][1] is not None:
            raise HeaderError('cannot parse the declarator %r' % stmt.strip())
        return items[0][0], ctype(const, base, ptr, stmt, **kw)

    def define(m):
        constants[m.group(1)] = integer(m.group(2), m.group(0))

    def directive(m):
        raise HeaderError('no rule for the directive %r' % m.group(0).strip())

    def enum(m):
        for item in m.group(1).split(','):
            e = re.fullmatch(r'\s*(\w+)\s*=\s*(-?\d+)\s*', item)
            if not e:
                raise HeaderError('cannot parse the enumerator %r' % item.strip())
            constants[e.group(1)] = int(e.group(2))

    def struct(m):
        name, fields = m.group(1), []
        if m.group(3) != name or name in structs:
            raise HeaderError('struct %s is typedef\'d as %s, or twice' % (name, m.group(3)))
        for stmt in filter(str.strip, m.group(2).split(';')):
            const, base, ptr, items = declare(stmt)
            t = ctype(const, base, ptr, stmt, member=True)
            fields += [(n, t if bound is None else t * bound) for n, bound in items]
        structs[name] = fields
        classes[name] = type(name, (C.Structure,), {'_fields_': fields})

    def prototype(m):
        name, res = one(m.group(1), ret=True)
        params = [] if m.group(2).strip() == 'void' else m.group(2).split(',')
        if name in functions:
            raise HeaderError('%s is declared twice' % name)
        functions[name] = (res, [one(p)[1] for p in params])

    text = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
    for pattern, handler, flags in (
            [(p, None, re.M) for p in _FRAME] +
            [(r'^#define[ \t]+(\w+)[ \t]+(.*?)[ \t]*$', define, re.M),
             (r'^[ \t]*#.*$', directive, re.M),
             (r'typedef\s+void\s*\*\s*(\w+)\s*;', lambda m: handles.append(m.group(1)), 0),
             (r'enum\s+\w+\s*\{([^{}]*)\}\s*;', enum, 0),
             (r'typedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*(\w+)\s*;', struct, 0),
             (r'([^;{}()]+)\(([^()]*)\)\s*;', prototype, 0)]):
        text = re.sub(pattern, lambda m: (handler and handler(m)) or ' ', text, flags=flags)
    if text.strip():
        raise HeaderError('no rule for this part of the header: %r' % ' '.join(text.split())[:200])
    names = {'structs': tuple(structs), 'functions': tuple(functions),
             'constants': tuple(constants)}
    return Abi(structs, functions, constants, names, tuple(handles), classes)
