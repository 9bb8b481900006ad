"""ctypes binding of libeventclip_hip.so, derived at import from include/eventclip_hip.h.

The header is the only statement of the C ABI.  ``read_header`` turns it into ``ABI_VERSION``, every ``EC_*`` enumerator
as a module-level int, one ``ctypes.Structure`` per ``typedef struct`` (``ec_gemm_args`` -> ``EcGemmArgs``) and
``SIGNATURES[name] = (restype, argtypes)`` for every ``EC_API`` prototype.  It knows the declaration forms the header
uses and raises, naming the line, on anything else: a declaration it cannot read stops the import, it is never skipped.

There is no CPU fallback: if the library is missing or no MI355X is visible the
callers raise.  torch is used only to own device memory and streams.
"""
import ctypes
import math
import os
import re

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(_HERE), 'include', 'eventclip_hip.h')      # where build.py takes INCLUDE from
# EVENTCLIP_HIP_LIB: tools/ point it at libeventclip_hip_diag.so (python -m eventclip_amd.build --diag),
# the build whose ec_gemm also has the stamp / timeline / timing-experiment variants
LIB_PATH = os.environ.get('EVENTCLIP_HIP_LIB') or os.path.join(_HERE, 'libeventclip_hip.so')
DIAG_LIB_PATH = os.path.join(_HERE, 'libeventclip_hip_diag.so')

c_void_p, c_int, c_long, c_double, c_float = (ctypes.c_void_p, ctypes.c_int, ctypes.c_long,
                                              ctypes.c_double, ctypes.c_float)


class HeaderError(ValueError):
    """The header holds something ``read_header`` does not know how to bind."""


_SCALARS = {'int': c_int, 'long': c_long, 'float': c_float, 'double': c_double, 'char': ctypes.c_char,
            'size_t': ctypes.c_size_t, 'uint8_t': ctypes.c_uint8, 'uint32_t': ctypes.c_uint32,
            'uint64_t': ctypes.c_uint64, 'int32_t': ctypes.c_int32, 'int64_t': ctypes.c_int64, 'ec_stream_t': c_void_p}
_SPACE = re.compile(r'\s*')
_COMMENT = re.compile(r'/\*.*?\*/|//[^\n]*', re.S)
_PREPROCESSOR = re.compile(r'^[ \t]*#(?:[^\n]*\\\n)*[^\n]*', re.M)              # a # line and its \ continuations
_VERSION = re.compile(r'^[ \t]*#[ \t]*define[ \t]+EC_ABI_VERSION[ \t]+(\d+)[ \t]*$', re.M)
_FRAME = re.compile(r'extern\s+"C"\s*\{|\}|typedef\s+void\s*\*\s*ec_stream_t\s*;')
_ENUM = re.compile(r'enum\s*\{([^{}]*)\}\s*;')
_STRUCT = re.compile(r'typedef\s+struct\s*\{([^{}]*)\}\s*(\w+)\s*;')
_PROTO = re.compile(r'EC_API\s+([^;()]*?)(\w+)\s*\(([^()]*)\)\s*;')
_ENUMERATOR = re.compile(r'(\w+)(?:\s*=\s*(-?\d+))?')
_DECLARATION = re.compile(r'(EC_DEVICE\s+)?(?:const\s+)?(\w+)\b\s*(.*)', re.S)  # [EC_DEVICE] [const] base type, declarators
_DECLARATOR = re.compile(r'(\*?)\s*(\w+)\s*(?:\[\s*(\d+)\s*\])?')               # [*] name [[literal]]


def read_header(text, filename='eventclip_hip.h'):
    """The header's text -> (abi_version, {EC_*: int}, {'EcName': Structure subclass}, {'ec_name': (restype, argtypes)});
    ``filename`` is the name its errors go under.

    Pointers: ``char *`` is ``c_char_p``; a pointer to a header struct is ``POINTER(thatStruct)`` unless the parameter
    is marked EC_DEVICE (an array in device memory: the caller passes its address); every other pointer, and an array
    parameter, is ``c_void_p``."""
    def blank(m):                                   # to a space and its newlines, so that what follows keeps its line
        return ' ' + '\n' * m.group().count('\n')

    def fail(pos, why):
        raise HeaderError(f'{filename}:{text.count(chr(10), 0, pos) + 1}: {why}')

    def parts(m, group, sep):
        """The sep-separated parts of a match's group, stripped, each with its position in the text."""
        pos = m.start(group)
        for part in m.group(group).split(sep):
            yield part.strip(), pos + len(part) - len(part.lstrip())
            pos += len(part) + 1

    def declaration(s, pos, param):
        """'[EC_DEVICE] [const] type declarator, ...' -> [(name, ctype)]; a parameter has one declarator."""
        m = _DECLARATION.fullmatch(s)
        device, base, declarators = m.groups() if m else (None, None, '')
        out = []
        for d in declarators.split(','):
            dm = _DECLARATOR.fullmatch(d.strip())
            if not dm or (device and not (param and dm[1] and base in by_c_name)):
                fail(pos, f'cannot read the declaration {s!r}')
            star, name, n = dm[1], dm[2], int(dm[3]) if dm[3] else None
            known = by_c_name.get(base) or _SCALARS.get(base)
            if known is None and not (base == 'void' and star):
                fail(pos, f'unknown type {base!r} in {s!r}')
            if star and n is None or param and n:                               # a pointer; an array parameter is one
                t = ctypes.c_char_p if base == 'char' else \
                    ctypes.POINTER(known) if base in by_c_name and not device else c_void_p
            elif star:                                                          # an array of pointers (a field)
                t = c_void_p * n
            else:
                t = known * n if n else known
            out.append((name, t))
        return out

    text = _COMMENT.sub(blank, text)
    version = _VERSION.search(text)
    if not version:
        fail(0, 'no #define EC_ABI_VERSION <number>')
    text = _PREPROCESSOR.sub(blank, text)
    constants, by_c_name, signatures = {}, {}, {}

    def enum(m):
        value = -1
        for e, pos in parts(m, 1, ','):
            em = _ENUMERATOR.fullmatch(e)
            if not em:
                if e == '' and pos >= m.end(1):                                 # the comma behind the last enumerator
                    continue
                fail(pos, f'cannot read the enumerator {e!r}')
            value = constants[em[1]] = int(em[2]) if em[2] else value + 1

    def struct(m):
        fields = []
        for f, pos in parts(m, 1, ';'):
            if f == '' and pos >= m.end(1):                                     # behind the last field's semicolon
                continue
            fields += declaration(f, pos, False)
        by_c_name[m[2]] = type(''.join(w.capitalize() for w in m[2].split('_')), (ctypes.Structure,), {'_fields_': fields})

    def proto(m):
        res = declaration(m[1] + ' _', m.start(1), True)[0][1]                  # the return type, as a nameless parameter
        args = [] if m[3].strip() == 'void' else [declaration(p, pos, True)[0][1] for p, pos in parts(m, 3, ',')]
        signatures[m[2]] = (res, args)

    pos, forms = 0, ((_FRAME, lambda m: None), (_ENUM, enum), (_STRUCT, struct), (_PROTO, proto))
    while True:
        pos = _SPACE.match(text, pos).end()
        if pos == len(text):
            break
        for rx, take in forms:
            m = rx.match(text, pos)
            if m:
                take(m)
                pos = m.end()
                break
        else:
            fail(pos, 'not a declaration form this reader knows (enum { }, typedef struct { } name, EC_API prototype)')
    for word, parsed in (('typedef\\s+struct', by_c_name), ('EC_API', signatures)):
        found = len(re.findall(rf'\b{word}\b', text))
        if found != len(parsed):
            fail(0, f'{found} `{word}` in the text, {len(parsed)} distinct declarations read')
    return int(version[1]), constants, {t.__name__: t for t in by_c_name.values()}, signatures


# ABI_VERSION (EC_ABI_VERSION), EC_F16 ..., EcGemmArgs ..., SIGNATURES: name -> (restype, argtypes)
with open(HEADER) as _f:
    ABI_VERSION, _constants, _structs, SIGNATURES = read_header(_f.read())
globals().update(_constants)
globals().update(_structs)

BLOCK_GRAD_FIELDS = tuple(n for n, _ in _structs['EcBlockGrads']._fields_)
# ec_gemm_args / ec_*_weights .activation, by the config's name for it (cfg['activation'])
ACTIVATIONS = {'quick_gelu': _constants['EC_ACT_QUICK_GELU'], 'gelu': _constants['EC_ACT_GELU']}


def activation_code(name):
    """cfg['activation'] (None = the default, QuickGELU) -> EC_ACT_*; anything else raises."""
    if name is None:
        return ACTIVATIONS['quick_gelu']
    if name not in ACTIVATIONS:
        raise ValueError(f"unknown activation {name!r}: one of {sorted(ACTIVATIONS)}")
    return ACTIVATIONS[name]


_lib = None
_bound = {}                 # side header's file name -> what bind_header read from it


class HipLibraryError(RuntimeError):
    pass


def _set_types(handle, signatures):
    for name, (res, args) in signatures.items():
        fn = getattr(handle, name)
        fn.restype = res
        fn.argtypes = args


def bind_header(filename):
    """A side header, include/``filename`` -> (constants, structs, signatures), read as the main header is; its
    ``#include "eventclip_hip.h"`` stands for what the reader wants from that header, the version.  The entries it
    declares are typed on the library's handle when ``lib()`` loads it, or here if it is loaded already: ``launch`` and
    ``getattr(lib(), name)`` find them typed whoever asks first.  Binding a header again returns what the first time read."""
    if filename not in _bound:
        with open(os.path.join(os.path.dirname(HEADER), filename)) as f:
            text = f.read().replace('#include "eventclip_hip.h"', f'#define EC_ABI_VERSION {ABI_VERSION}')
        _bound[filename] = read_header(text, filename)[1:]
        if _lib is not None:
            _set_types(_lib, _bound[filename][2])
    return _bound[filename]


def lib():
    """Load the library once.  Raises HipLibraryError when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise HipLibraryError(
                f'{LIB_PATH} is missing: build it with `python -m eventclip_amd.build` '
                '(hipcc --offload-arch=gfx950).  eventclip_amd has no CPU fallback.')
        # One HIP runtime per process: torch bundles its own libamdhip64 (soname
        # libamdhip64.so.7).  Load it first so that this library's NEEDED entry
        # binds to the same runtime instead of pulling a second copy from
        # /opt/rocm, whose streams and device state torch would not share.
        bundled = os.path.join(os.path.dirname(torch.__file__), 'lib', 'libamdhip64.so')
        if os.path.exists(bundled):
            ctypes.CDLL(bundled, mode=ctypes.RTLD_GLOBAL)
        handle = ctypes.CDLL(LIB_PATH)
        _set_types(handle, SIGNATURES)
        for _, _, signatures in _bound.values():
            _set_types(handle, signatures)
        # the header this module read against the one the library was built from (include/eventclip_hip.h, EC_ABI_CHECK)
        rc = handle.ec_abi_check(ABI_VERSION, *(ctypes.sizeof(_structs[t]) for t in (
            'EcGemmArgs', 'EcBlockWeights', 'EcVitWeights', 'EcTextWeights', 'EcEventsParams', 'EcAdapterWeights')))
        if rc != 0:
            raise HipLibraryError(f'{LIB_PATH}: {handle.ec_last_error().decode()} ({HEADER} states ABI '
                                  f'{ABI_VERSION}; rebuild with `python -m eventclip_amd.build`)')
        _lib = handle
    return _lib


def check(rc, what=''):
    if rc != 0:
        msg = lib().ec_last_error()
        raise RuntimeError(f'{what or "libeventclip_hip"} failed ({rc}): '
                           f'{msg.decode() if msg else ""}')


def require_gpu():
    """The device every op runs on; raises when there is none."""
    if not torch.cuda.is_available():
        raise HipLibraryError('eventclip_amd needs an MI355X (gfx950) device: '
                              'torch.cuda.is_available() is False and there is no CPU fallback.')
    return torch.device('cuda', torch.cuda.current_device())


def stream_ptr():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    """Device pointer of a torch tensor (None -> NULL), for tests and tools that call the ABI directly; code in this
    package passes the tensor itself to ``launch``, which also keeps it alive over the call."""
    if t is None:
        return None
    return ctypes.c_void_p(t.data_ptr())


_PLAIN = frozenset({int, float, type(None)})


def launch(name, *args):
    """Call the stream-taking entry ``name`` on torch's current stream and raise under its name when it fails.
    A tensor goes as its device pointer, None as NULL, a ctypes Structure by reference, anything else (a ``byref``,
    a scalar, a host address) as it is.  ``args`` holds every tensor until the call has returned, so temporaries are
    safe to pass; the arrays behind a struct's pointer FIELDS are raw addresses and stay the caller's to keep."""
    conv = []
    for a in args:
        if type(a) in _PLAIN:                     # most of any argument list: told by exact type, before the isinstance tests
            pass
        elif isinstance(a, torch.Tensor):
            a = a.data_ptr()
        elif isinstance(a, ctypes.Structure):
            a = ctypes.byref(a)
        conv.append(a)
    check(getattr(lib(), name)(*conv, stream_ptr()), name)


def scratch(nbytes, device):
    """A fresh uint8 device buffer of at least ``nbytes`` (never empty: the kernels want a real pointer)."""
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)


class Scratch:
    """Grow-only uint8 device buffer, reused from call to call: ``get`` reallocates only for more bytes or another
    device, and drops the old block first so the two never coexist.  ``device`` must carry its index (``require_gpu()``,
    ``tensor.device``): a bare ``torch.device('cuda')`` never equals the buffer's device and would reallocate every call."""

    def __init__(self):
        self.buf = None

    def get(self, nbytes, device):
        if self.buf is None or self.buf.numel() < nbytes or self.buf.device != device:
            self.buf = None
            self.buf = torch.empty((int(nbytes),), dtype=torch.uint8, device=device)
        return self.buf


def device_table(items):
    """ctypes array of structs -> device copy (uint8 CUDA tensor) for the batched kernels' item tables."""
    return torch.from_numpy(np.frombuffer(items, dtype=np.uint8).copy()).cuda()


def flat_views(shapes, device, min_numel=0):
    """{name: shape} -> (flat, {name: view}): one zeroed fp32 buffer (a single all-reduce / unscale covers it) and a
    view of it per name, laid out in mapping order; views[name].storage_offset() is the name's offset in ``flat``."""
    flat = torch.zeros((max(sum(math.prod(s) for s in shapes.values()), min_numel),), dtype=torch.float32, device=device)
    views, off = {}, 0
    for name, shape in shapes.items():
        views[name] = flat[off:off + math.prod(shape)].view(tuple(shape))
        off += math.prod(shape)
    return flat, views


def profile_begin():
    check(lib().ec_profile_begin(), 'ec_profile_begin')


def profile_end():
    """-> list of dicts (name, launches, total_ms, flops, bytes), one per kernel symbol."""
    arr = (_structs['EcProfileEntry'] * 32)()
    n = c_int(0)
    check(lib().ec_profile_end(arr, 32, ctypes.byref(n)), 'ec_profile_end')
    return [dict(name=arr[i].name.decode(), launches=int(arr[i].launches),
                 total_ms=float(arr[i].total_ms), flops=float(arr[i].flops),
                 bytes=float(arr[i].bytes)) for i in range(n.value)]
