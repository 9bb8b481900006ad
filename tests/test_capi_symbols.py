"""The C-ABI library loads on a CPU-only box and exports every symbol the header declares, and the ctypes bindings that
eventclip_amd/_lib.py derives from the header are what the host compiler makes of the same header."""
import ctypes
import os
import re

from eventclip_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_symbols():
    text = open(os.path.join(ROOT, 'include', 'eventclip_hip.h')).read()
    return sorted(set(re.findall(r'EC_API\s+[\w\s\*]+?\b(ec_\w+)\s*\(', text)))


def test_library_built_and_exports_header():
    syms = header_symbols()
    assert len(syms) >= 4
    assert os.path.exists(_lib.LIB_PATH), 'run `python -m eventclip_amd.build`'
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for s in syms:
        assert hasattr(handle, s), f'{s} declared in include/eventclip_hip.h but not exported'


def _compile_and_run(tmp_path, compiler, flags, name, source):
    """The output lines of `source`, compiled by the host compiler against include/ (nothing of the library is linked)."""
    import shutil
    import subprocess
    import pytest
    exe = shutil.which(os.environ.get(*compiler))
    if exe is None:
        pytest.skip(f'no {compiler[1]}')
    src = tmp_path / name
    src.write_text(source)
    r = subprocess.run([exe, *flags, '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(tmp_path / 'prog')],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return subprocess.run([str(tmp_path / 'prog')], capture_output=True, text=True, check=True).stdout.splitlines()


def _structs():
    """{C name: class} of every Structure the binding derived (EcBlockWeightsT -> ec_block_weights_t)."""
    return {re.sub(r'(?<!^)(?=[A-Z])', '_', k).lower(): v for k, v in vars(_lib).items()
            if isinstance(v, type) and issubclass(v, ctypes.Structure) and v is not ctypes.Structure}


def test_layout_and_constants_match_the_compiler(tmp_path):
    """The bindings come from a regex reader of the header; the host C compiler reads the same header and says what it
    means: sizeof of all 25 structs, offsetof and sizeof of every field, the value of every enumerator, EC_ABI_VERSION.
    Nothing may be missing on either side: the names are counted in the header with other patterns than the reader's."""
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'eventclip_hip.h')).read(), flags=re.S)
    structs = _structs()
    constants = {k: v for k, v in vars(_lib).items() if k.startswith('EC_') and isinstance(v, int)}
    assert sorted(structs) == sorted(re.findall(r'\}\s*(ec_\w+)\s*;', text)) and len(structs) == 25
    assert sorted(constants) == sorted(n for body in re.findall(r'\benum\s*\{(.*?)\}', text, re.S)
                                       for n in re.findall(r'\bEC_\w+', body)) and len(constants) == 89
    body, want = ['printf("V %d\\n", EC_ABI_VERSION);'], [f'V {_lib.ABI_VERSION}']
    for name, value in constants.items():
        body.append(f'printf("E {name} %d\\n", (int){name});')
        want.append(f'E {name} {value}')
    for c_name, cls in structs.items():
        body.append(f'printf("S {c_name} %zu\\n", sizeof({c_name}));')
        want.append(f'S {c_name} {ctypes.sizeof(cls)}')
        for field, _ in cls._fields_:
            body.append(f'printf("F {c_name} {field} %zu %zu\\n", offsetof({c_name}, {field}), '
                        f'sizeof((({c_name} *)0)->{field}));')
            want.append(f'F {c_name} {field} {getattr(cls, field).offset} {getattr(cls, field).size}')
    got = _compile_and_run(tmp_path, ('CC', 'cc'), [], 'layout.c',
                           '#include <stdio.h>\n#include <stddef.h>\n#include "eventclip_hip.h"\nint main(void) {\n'
                           + '\n'.join(body) + '\nreturn 0; }\n')
    assert got == want, [(g, w) for g, w in zip(got, want) if g != w][:10]


SIGNATURE_PROGRAM = r'''#include <cstdio>
#include <type_traits>
#include "eventclip_hip.h"
template <class T> void kind() {
    if constexpr (std::is_void_v<T>) std::printf(" v0");
    else if constexpr (std::is_pointer_v<T>) std::printf(" p%zu", sizeof(T));
    else if constexpr (std::is_floating_point_v<T>) std::printf(" f%zu", sizeof(T));
    else if constexpr (std::is_integral_v<T>) std::printf(" %c%zu", std::is_signed_v<T> ? 'i' : 'u', sizeof(T));
    else std::printf(" ?%zu", sizeof(T));
}
template <class R, class... A> void sig(const char *name, R (*)(A...)) {
    std::printf("%s", name);
    kind<R>();
    (kind<A>(), ...);
    std::printf("\n");
}
int main() {
CALLS    return 0;
}
'''


def _kind(t):
    """restype / argtype -> what SIGNATURE_PROGRAM prints for the C type: v0, p8, f4 / f8, i<bytes> / u<bytes>."""
    if t is None:
        return 'v0'
    if issubclass(t, ctypes._Pointer) or t in (ctypes.c_void_p, ctypes.c_char_p):
        return f'p{ctypes.sizeof(t)}'
    if t in (ctypes.c_float, ctypes.c_double):
        return f'f{ctypes.sizeof(t)}'
    return ('i' if t(-1).value < 0 else 'u') + str(ctypes.sizeof(t))


def test_signatures_match_the_compiler(tmp_path):
    """Every prototype of the header taken apart by the host C++ compiler (template deduction on decltype(&ec_xxx),
    unevaluated: nothing links against the library or HIP): the arity and, for the return type and each parameter, the
    kind (pointer, integral, floating, void), the size and an integral's signedness, against restype / argtypes of all
    98 SIGNATURES entries.  An int bound as long, a float bound as double or a missing argument differs here."""
    names = header_symbols()
    assert sorted(_lib.SIGNATURES) == names and len(names) == 98
    calls = ''.join(f'    sig("{n}", static_cast<decltype(&{n})>(nullptr));\n' for n in names)
    got = _compile_and_run(tmp_path, ('CXX', 'c++'), ['-std=c++17'], 'signatures.cpp',
                           SIGNATURE_PROGRAM.replace('CALLS', calls))
    want = [' '.join([n, _kind(_lib.SIGNATURES[n][0])] + [_kind(a) for a in _lib.SIGNATURES[n][1]]) for n in names]
    assert got == want, [(g, w) for g, w in zip(got, want) if g != w][:10]


def test_struct_pointers_are_typed_and_device_arrays_are_addresses():
    """The pointer rules, which the compiler cannot tell apart: a host struct goes by POINTER(itsStruct), an EC_DEVICE array
    of structs by its address; BLOCK_GRAD_FIELDS is ec_block_grads' fields."""
    assert _lib.SIGNATURES['ec_gemm'][1][0] is ctypes.POINTER(_lib.EcGemmArgs)
    assert _lib.SIGNATURES['ec_profile_end'][1][0] is ctypes.POINTER(_lib.EcProfileEntry)
    assert dict(_lib.EcVitWeights._fields_)['blocks'] is ctypes.POINTER(_lib.EcBlockWeights)
    for name, i in (('ec_events_to_frames', 7), ('ec_events_to_frames_packed', 7), ('ec_randaugment', 5),
                    ('ec_pack_weight16_batched', 0), ('ec_fingerprint_batched', 0), ('ec_lora_merge_batched', 0),
                    ('ec_lora_grad_batched', 0), ('ec_adam_step_multi', 0)):
        assert _lib.SIGNATURES[name][1][i] is ctypes.c_void_p, name
    assert _lib.BLOCK_GRAD_FIELDS == tuple(n for n, _ in _lib.EcBlockGrads._fields_) and len(_lib.BLOCK_GRAD_FIELDS) == 12


SNIPPET = '#define EC_ABI_VERSION 7\n#define EC_API\ntypedef void *ec_stream_t;\n'      # lines 1 - 3 of every case below


def test_reader_reads_the_forms_the_header_uses():
    version, constants, structs, signatures = _lib.read_header(SNIPPET + '''
enum { EC_A = 2, EC_B, /* implicit */ EC_C = -4, EC_D, };
typedef struct { const float *p /* note */, *q; uint8_t rgb[3]; const void *tab[4]; } ec_inner;
typedef struct { int n; ec_inner one, two[2]; const ec_inner *more; } ec_outer_t;
EC_API const char *ec_name(void);
EC_API size_t ec_f(const ec_outer_t *w, EC_DEVICE const ec_inner *items, const uint8_t fill[3], float x /* why */,
                   ec_stream_t stream);
''')
    assert version == 7 and constants == dict(EC_A=2, EC_B=3, EC_C=-4, EC_D=-3)
    inner, outer = structs['EcInner'], structs['EcOuterT']
    assert inner._fields_ == [('p', ctypes.c_void_p), ('q', ctypes.c_void_p), ('rgb', ctypes.c_uint8 * 3),
                              ('tab', ctypes.c_void_p * 4)]
    assert outer._fields_ == [('n', ctypes.c_int), ('one', inner), ('two', inner * 2), ('more', ctypes.POINTER(inner))]
    assert signatures == {'ec_name': (ctypes.c_char_p, []),
                          'ec_f': (ctypes.c_size_t, [ctypes.POINTER(outer), ctypes.c_void_p, ctypes.c_void_p,
                                                     ctypes.c_float, ctypes.c_void_p])}


def test_reader_refuses_what_it_cannot_read():
    """A declaration the reader does not know stops it under the line's number; nothing is skipped."""
    import pytest
    for bad, line, why in (
            ('typedef struct { int n;\n float16_t x; } ec_a;', 5, 'unknown type'),
            ('typedef struct { ec_later *p; } ec_a;', 4, 'unknown type'),
            ('typedef struct { void v; } ec_a;', 4, 'unknown type'),
            ('typedef struct { int flags : 3; } ec_a;', 4, 'cannot read'),
            ('typedef struct { unsigned int n; } ec_a;', 4, 'cannot read'),
            ('typedef struct { float **pp; } ec_a;', 4, 'cannot read'),
            ('typedef struct { int (*cb)(int); } ec_a;', 4, 'cannot read'),
            ('typedef struct { int n[EC_N]; } ec_a;', 4, 'cannot read'),
            ('typedef struct { EC_DEVICE int *p; } ec_a;', 4, 'cannot read'),
            ('\ntypedef struct { union { int i; float f; } u; } ec_a;', 5, 'not a declaration form'),
            ('typedef struct tag { int n; } ec_a;', 4, 'not a declaration form'),
            ('EC_API int ec_f(int (*cb)(int), ec_stream_t stream);', 4, 'not a declaration form'),
            ('EC_API int ec_f(int n,\n int, ec_stream_t stream);', 5, 'cannot read'),
            ('EC_API int ec_f(int n, ...);', 4, 'cannot read'),
            ('EC_API void ec_f(int n);', 4, 'unknown type'),
            ('EC_API int ec_f(int n)\nEC_API int ec_g(void);', 4, 'not a declaration form'),
            ('enum { EC_A = 1 << 2 };', 4, 'cannot read the enumerator'),
            ('int ec_global;', 4, 'not a declaration form'),
            ('typedef struct { int a; } ec_a;\ntypedef struct { int b; } ec_a;', 1, '2 `typedef.*1 distinct'),
            ('EC_API int ec_f(void);\nEC_API int ec_f(int n);', 1, '2 `EC_API` in the text, 1 distinct')):
        with pytest.raises(_lib.HeaderError, match=rf'eventclip_hip\.h:{line}: .*{why}'):
            _lib.read_header(SNIPPET + bad)
    with pytest.raises(_lib.HeaderError, match='EC_ABI_VERSION'):
        _lib.read_header('enum { EC_A = 0 };')


def test_side_headers_are_bound_whatever_the_call_order(monkeypatch):
    """Importing vis binds the three side headers; every entry they declare is then typed on the handle ``lib()`` returns,
    whether the library was loaded before the binding or is loaded after it, and with no call in between.  Binding a
    header again changes nothing; a side header's errors carry its own name; _lib's own tables stay the main header's."""
    import pytest
    from eventclip_amd import vis
    tables = {'eventclip_time_surface.h': vis.SURFACE_SIGNATURES, 'eventclip_voxel_grid.h': vis.VOXEL_SIGNATURES,
              'eventclip_denoise.h': vis.DENOISE_SIGNATURES}
    assert [os.path.basename(h) for h in (vis.SURFACE_HEADER, vis.VOXEL_HEADER, vis.DENOISE_HEADER)] == list(tables)
    assert all(len(t) >= 2 for t in tables.values()) and not any(set(t) & set(_lib.SIGNATURES) for t in tables.values())

    def typed(handle):
        for table in tables.values():
            for name, (res, args) in table.items():
                fn = getattr(handle, name)
                assert fn.restype is res and list(fn.argtypes) == args, name
    typed(_lib.lib())
    monkeypatch.setattr(_lib, '_lib', None)                    # ... and on a handle loaded after the binding
    fresh = _lib.lib()
    typed(fresh)
    for filename, table in tables.items():                     # again, now with the library loaded: the very same tables
        constants, structs, signatures = _lib.bind_header(filename)
        assert signatures is table and set(structs) and all(k.startswith('EC_') for k in constants)
        assert not set(structs) & set(vars(_lib)) and not set(constants) & set(vars(_lib))
    typed(fresh)
    assert fresh.ec_voxel_grid_bands(100, 120, 3) == 1 and fresh.ec_denoise_bands(37, 53, 1) == 1
    with pytest.raises(_lib.HeaderError, match=r'eventclip_side\.h:4: .*not a declaration form'):
        _lib.read_header(SNIPPET + 'int ec_global;', 'eventclip_side.h')


def test_version_and_error_string():
    lib = _lib.lib()
    assert lib.ec_version() == _lib.ABI_VERSION == header_abi_version()
    assert isinstance(lib.ec_last_error(), bytes)


def header_abi_version():
    text = open(os.path.join(ROOT, 'include', 'eventclip_hip.h')).read()
    return int(re.search(r'#define\s+EC_ABI_VERSION\s+(\d+)', text).group(1))


def test_abi_check_rejects_older_headers_and_short_structs():
    """ec_gemm_args / ec_vit_weights grew and ec_classify changed its argument list while ec_version() stayed
    100.  ABI 600: ec_abi_check compares the caller's header version and struct sizes with the library's (the loader
    of eventclip_amd/_lib.py calls it with the sizes of its ctypes structs); a caller built against an older header is refused with a
    message, and the old ec_classify name is a stub that returns an error code."""
    lib = _lib.lib()
    sizes = [ctypes.sizeof(t) for t in (_lib.EcGemmArgs, _lib.EcBlockWeights, _lib.EcVitWeights, _lib.EcTextWeights,
                                        _lib.EcEventsParams, _lib.EcAdapterWeights)]
    assert lib.ec_abi_check(_lib.ABI_VERSION, *sizes) == 0
    assert lib.ec_abi_check(100, *sizes) == _lib.EC_ERR_INVALID and b'ABI 100' in lib.ec_last_error()
    short = list(sizes)
    short[0] = 176                                   # ec_gemm_args as round 4 had it (no A_lo / W_lo)
    assert lib.ec_abi_check(_lib.ABI_VERSION, *short) == _lib.EC_ERR_INVALID and b'ec_gemm_args' in lib.ec_last_error()
    short = list(sizes)
    short[2] -= 8                                    # ec_vit_weights without its last field
    assert lib.ec_abi_check(_lib.ABI_VERSION, *short) == _lib.EC_ERR_INVALID and b'ec_vit_weights' in lib.ec_last_error()
    assert lib.ec_classify() == _lib.EC_ERR_UNSUPPORTED and b'ec_classify_v2' in lib.ec_last_error()


def test_struct_layout_matches_header():
    assert ctypes.sizeof(_lib.EcFrameStats) == 40
    assert ctypes.sizeof(_lib.EcEventsParams) == 80
    assert ctypes.sizeof(_lib.EcGemmArgs) == 248     # (+ A_lo, W_lo: round 5; + the four e4m3 operands and their exponents: round 6)


def test_attention_kernels_have_no_unpadded_asm_hazards():
    """csrc/attention.hip updates its accumulators with inline-asm MFMAs, whose hazards hipcc does not pad
    (cdna_hip_programming.md 5.7): tools/check_attn_isa.py compiles the file and scans every product kernel for a
    vector write right in front of an unpadded asm MFMA and for accumulator copies in the key-block loops."""
    import os
    import shutil
    import sys
    import pytest
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip('no hipcc')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, 'tools'))
    import check_attn_isa
    assert check_attn_isa.main() == 0


def test_gemm_kernels_keep_their_schedule_and_have_no_scratch():
    """csrc/gemm.hip's persistent kernel issues the MFMAs of a phase between `s_setprio 1` / `s_setprio 0`, closed by barriers,
    and counts its vmcnt waits: tools/check_gemm_isa.py compiles the file and checks every instantiation for scratch, for an
    empty matrix-pipe slot (round 6: hipcc had sunk the e4m3 MFMAs of a phase in front of the next phase's) and for phases
    whose MFMA count is neither 32 (16-bit) nor 16 (e4m3)."""
    import shutil
    import sys
    import pytest
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip('no hipcc')
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import check_gemm_isa
    assert check_gemm_isa.main() == 0


def test_diagnostic_build_of_gemm_and_attention_compiles():
    """The diagnostic build (python -m eventclip_amd.build --diag) keeps its instrumentation of the shipped kernels -- the
    GEMM's timeline / clock-stamp variants and MFMA rate probe, the attention's phase stamps -- and nothing else builds it:
    compile both files device-only with its flags, so that the instrumentation cannot rot unseen."""
    import shutil
    import subprocess
    import tempfile
    import pytest
    from eventclip_amd import build
    if not (os.path.exists(build.HIPCC) or shutil.which(build.HIPCC)):
        pytest.skip('no hipcc')
    with tempfile.TemporaryDirectory() as tmp:
        procs = [(f, subprocess.Popen([build.HIPCC] + build.FLAGS + build.DIAG_FLAGS +
                                      ['--cuda-device-only', '-c', os.path.join(build.CSRC, f), '-o', os.path.join(tmp, f + '.o')],
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
                 for f in ('gemm.hip', 'attention.hip')]
        for f, p in procs:
            out, _ = p.communicate()
            assert p.returncode == 0, f'{f} (diagnostic build):\n{out}'
