"""The hand-written ctypes layer against include/ndcn_hip.h, compared by the compiler (tests/test_cabi.py compares the NAMES only).

A C++17 translation unit is generated into a temporary directory: one `decltype(&name)` per prototype of `_lib.SIGNATURES`, fed to a
variadic template that prints the return kind and every parameter's kind (void, ptr, i4 / i8, u4 / u8, f4 / f8); `sizeof` of the six
structs the binding mirrors and `offsetof` / `sizeof` / kind of every field, the field names taken from the ctypes `_fields_` (a field
missing on either side is a compile error or a difference); and the value of every NDCN_* macro whose name `_lib.py` restates.  It is
compiled for the host alone against the header alone, never linked against the library, and its output is compared with the same
description derived from ctypes.  A `c_int` written for an `int64_t`, a `c_float` for a `double` or two same-sized fields in swapped
order all load and mostly run; here each is a named difference.  The partial binding of examples/ndcn_hip_binding.py is executed
against a recording stand-in for the library and held to the same description."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from ndcn_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, 'include')

# ctypes mirror -> the header's type; the blocks of ndcn_shard are an unnamed struct there
STRUCTS = [(_lib.CsrView, 'ndcn_csr'), (_lib.CsrHints, 'ndcn_csr_hints'), (_lib.DropoutDesc, 'ndcn_dropout'),
           (_lib.Dynamics, 'ndcn_dynamics'), (_lib.ShardBlock, 'std::remove_all_extents_t<decltype(ndcn_shard::blocks)>'),
           (_lib.ShardView, 'ndcn_shard'), (_lib.SolverDesc, 'ndcn_solver_desc')]

# the constants _lib.py restates: binding name -> header name.  Every name of these families that the header defines is compared.
CONSTANT_FAMILIES = ('F_', 'RK_', 'M_', 'PLAN_', 'PATH_', 'VJP_', 'DYN_', 'LIN_', 'RKB_', 'SPMM_', 'RKF_', 'READOUT_', 'SSR_')
CONSTANT_NAMES = ('OK', 'EINVAL', 'EHIP', 'ENONFINITE', 'EUNDERFLOW', 'EMAXSTEPS', 'ESTATE', 'ECAPACITY', 'ABI_VERSION')
# ... and these the header must define (the rest of a family may be the binding's own, like RK_NONE = 0)
REQUIRED = ('F_RELU', 'F_NO_GRAPH', 'F_NO_CONTROL', 'F_ACCUM', 'RK_COMBINE', 'RK_ERROR', 'RK_RK4', 'M_EULER', 'M_MIDPOINT', 'M_RK4',
            'M_DOPRI5', 'PLAN_NO_REC', 'PLAN_NO_STENCIL', 'PLAN_NO_TILE_ORDER', 'PLAN_NO_HUB', 'PLAN_EXTERNAL_SCRATCH', 'PLAN_ORDER_ONLY',
            'PLAN_NO_SWEEP', 'PLAN_FORCE_SWEEP', 'PATH_FUSED2', 'PATH_FUSED3', 'PATH_HUB', 'PATH_HALO', 'PATH_SWEEP', 'PATH_REC',
            'PATH_WIDE', 'PATH_SMALL', 'PATH_EXACT32', 'PATH_RANGE', 'PATH_DROP_EPI', 'PATH_DYN', 'PATH_MID', 'PATH_ABL', 'VJP_COMPOSED',
            'VJP_MID', 'VJP_ABL', 'DYN_HEAT', 'DYN_GENE', 'DYN_MUTUAL', 'EINVAL', 'EHIP', 'ABI_VERSION')


def kind(t):
    """void / ptr / i<bytes> / u<bytes> / f<bytes> of a ctypes type"""
    if t is None:
        return 'void'
    if issubclass(t, (ctypes._Pointer, ctypes._CFuncPtr)):
        return 'ptr'
    if issubclass(t, ctypes._SimpleCData):
        code = t._type_
        if code in 'PzZO':
            return 'ptr'
        if code in 'fdg':
            return 'f%d' % ctypes.sizeof(t)
        if code in 'bhilq':
            return 'i%d' % ctypes.sizeof(t)
        if code in 'BHILQ':
            return 'u%d' % ctypes.sizeof(t)
    return 'agg%d' % ctypes.sizeof(t)              # arrays and nested structs: compared by offset and size


def binding_constants(lib=_lib):
    names = [n for n in vars(lib) if (n.startswith(CONSTANT_FAMILIES) or n in CONSTANT_NAMES) and type(getattr(lib, n)) is int]
    return {n: getattr(lib, n) for n in names}


PRELUDE = r'''
#include "ndcn_hip.h"
#include <cstddef>
#include <cstdio>
#include <type_traits>
#include <utility>
template <class T> static void kind() {
    if constexpr (std::is_void_v<T>) std::printf(" void");
    else if constexpr (std::is_pointer_v<T>) std::printf(" ptr");
    else if constexpr (std::is_floating_point_v<T>) std::printf(" f%d", (int)sizeof(T));
    else if constexpr (std::is_enum_v<T>) kind<std::underlying_type_t<T>>();
    else if constexpr (std::is_integral_v<T>) std::printf(" %c%d", std::is_signed_v<T> ? 'i' : 'u', (int)sizeof(T));
    else std::printf(" agg%d", (int)sizeof(T));
}
template <class P> struct sig;                                      // (of the TYPE of &name alone: no symbol is referenced)
template <class R, class... A> struct sig<R (*)(A...)> {
    static void print(const char *name) { std::printf("F %s", name); kind<R>(); (kind<A>(), ...); std::printf("\n"); }
};
// the number of initializers the aggregate T takes (an array member counts once per element): a field of the header that the binding
// does not mirror moves no offset when it sits where padding would be - the count still differs
struct any_t { template <class T> operator T() const; };
template <class T, std::size_t... I> constexpr auto can(std::index_sequence<I...>, int) -> decltype(T{(void(I), any_t{})...}, bool()) { return true; }
template <class T, std::size_t... I> constexpr bool can(std::index_sequence<I...>, long) { return false; }
template <class T, std::size_t N = 0> constexpr std::size_t arity() {
    if constexpr (can<T>(std::make_index_sequence<N + 1>{}, 0)) return arity<T, N + 1>(); else return N;
}
#define FIELD(T, tag, f) do { std::printf("M %s %s %d %d", tag, #f, (int)offsetof(T, f), (int)sizeof(T::f)); \
                              kind<decltype(T::f)>(); std::printf("\n"); } while (0)
int main() {
'''


def generate(functions, structs, constants):
    src = [PRELUDE]
    for name in functions:
        src.append('    sig<decltype(&%s)>::print("%s");' % (name, name))
    for j, (cls, ctype) in enumerate(structs):
        src.append('    { using T%d = %s; std::printf("S %s %%d %%d\\n", (int)sizeof(T%d), (int)arity<T%d>());' % (j, ctype, cls.__name__, j, j))
        for field in cls._fields_:
            src.append('      FIELD(T%d, "%s", %s);' % (j, cls.__name__, field[0]))
        src.append('    }')
    for name in constants:
        src.append('#ifdef NDCN_%s\n    std::printf("C %s %%lld\\n", (long long)(NDCN_%s));\n#endif' % (name, name, name))
    src.append('    return 0;\n}\n')
    return '\n'.join(src)


def host_compiler():
    """the host C++ compiler of the build: what hipcc drives (ROCm's clang++), else the system's"""
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    rocm_clang = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), 'llvm', 'bin', 'clang++')
    for cxx in (os.environ.get('CXX'), rocm_clang, shutil.which('g++'), shutil.which('c++'), shutil.which('clang++')):
        if cxx and (os.path.exists(cxx) or shutil.which(cxx)):
            return cxx
    raise AssertionError('no host C++ compiler found')


def compile_and_run(source, tmp):
    """host-only compile (plain C++: no offload, no HIP headers), not linked against the library; returns (ok, output)"""
    path = os.path.join(str(tmp), 'probe.cpp')
    with open(path, 'w') as f:
        f.write(source)
    exe = os.path.join(str(tmp), 'probe')
    cc = subprocess.run([host_compiler(), '-x', 'c++', '-std=c++17', '-Wno-invalid-offsetof', '-I', INCLUDE, path, '-o', exe],
                        capture_output=True, text=True)
    if cc.returncode != 0:
        return False, cc.stderr
    return True, subprocess.run([exe], capture_output=True, text=True, check=True).stdout


def header_description(tmp, functions, structs, constants):
    ok, out = compile_and_run(generate(functions, structs, constants), tmp)
    assert ok, 'the probe does not compile against include/ndcn_hip.h:\n' + out[-3000:]
    funcs, sizes, fields, consts = {}, {}, {}, {}
    for line in out.splitlines():
        w = line.split()
        if w[0] == 'F':
            funcs[w[1]] = (w[2], w[3:])
        elif w[0] == 'S':
            sizes[w[1]] = (int(w[2]), int(w[3]))
        elif w[0] == 'M':
            fields[(w[1], w[2])] = (int(w[3]), int(w[4]), w[5])
        elif w[0] == 'C':
            consts[w[1]] = int(w[2])
    return funcs, sizes, fields, consts


def compare(lib, tmp):
    """every difference between the binding module `lib` and the header, as a list of sentences"""
    constants = binding_constants(lib)
    structs = [(getattr(lib, cls.__name__), ctype) for cls, ctype in STRUCTS]
    funcs, sizes, fields, consts = header_description(tmp, list(lib.SIGNATURES), structs, list(constants))
    said = []
    for name, (res, args) in lib.SIGNATURES.items():
        h_res, h_args = funcs[name]
        if kind(res) != h_res:
            said.append('%s: returns %s in the header, %s in the binding' % (name, h_res, kind(res)))
        if len(args) != len(h_args):
            said.append('%s: %d arguments in the header, %d in the binding' % (name, len(h_args), len(args)))
        for j, (a, h) in enumerate(zip(args, h_args)):
            if kind(a) != h:
                said.append('%s: argument %d is %s in the header, %s in the binding' % (name, j, h, kind(a)))
    for cls, _ in structs:
        nbytes, count = sizes[cls.__name__]
        if ctypes.sizeof(cls) != nbytes:
            said.append('%s: %d bytes in the header, %d in the binding' % (cls.__name__, nbytes, ctypes.sizeof(cls)))
        mirrored = sum(f[1]._length_ if issubclass(f[1], ctypes.Array) else 1 for f in cls._fields_)
        if mirrored != count:
            said.append('%s: %d fields (array elements counted) in the header, %d in the binding' % (cls.__name__, count, mirrored))
        for field in cls._fields_:
            d = getattr(cls, field[0])
            want = fields[(cls.__name__, field[0])]
            got = (d.offset, d.size, kind(field[1]))
            if got != want:
                said.append('%s.%s: (offset, size, kind) %s in the header, %s in the binding' % (cls.__name__, field[0], want, got))
    for name, v in constants.items():
        if name in consts and consts[name] != v:
            said.append('%s: %d in the header, %d in the binding' % (name, consts[name], v))
    for name in REQUIRED:
        if name not in consts or name not in constants:
            said.append('%s: not stated by both the header and the binding' % name)
    return said


def test_prototypes_struct_layouts_and_constants_agree_with_the_header(tmp_path):
    assert compare(_lib, tmp_path) == []


def test_a_field_the_header_lacks_does_not_compile(tmp_path):
    """the probe itself: a ctypes field with no counterpart in the header is a compile error, not a silent pass"""
    class Dynamics(ctypes.Structure):
        _fields_ = list(_lib.Dynamics._fields_) + [('extra', ctypes.c_int)]
    ok, err = compile_and_run(generate([], [(Dynamics, 'ndcn_dynamics')], []), tmp_path)
    assert not ok and 'extra' in err


# ---------------------------------------------------------------- examples/ndcn_hip_binding.py
class _Fn:
    def __init__(self, name):
        self.name = name

    def __call__(self, *args):
        return _lib.ABI_VERSION if self.name == 'ndcn_abi_version' else 0


class _Recorder:
    """stands in for ctypes.CDLL: hands out one attribute-recording callable per symbol"""
    def __init__(self, *args, **kw):
        self.fns = {}

    def __getattr__(self, name):
        if not name.startswith('ndcn_'):
            raise AttributeError(name)
        return self.fns.setdefault(name, _Fn(name))


def example_binding(path, monkeypatch):
    """(what the example sets: name -> {'restype': .., 'argtypes': ..}, the names it calls) - executed against the recorder"""
    import runpy
    made = []
    monkeypatch.setattr(ctypes, 'CDLL', lambda *a, **kw: made.append(_Recorder()) or made[-1])
    runpy.run_path(path)
    assert len(made) == 1
    text = open(path).read()
    called = set(re.findall(r'_lib\.(ndcn_\w+)\(', text))
    return {n: {k: v for k, v in vars(f).items() if k in ('restype', 'argtypes')} for n, f in made[0].fns.items()}, called


def compare_example(path, tmp, monkeypatch):
    set_, called = example_binding(path, monkeypatch)
    names = sorted(set(set_) | called)
    funcs, _, _, _ = header_description(tmp, names, [], [])
    said = []
    for name in names:
        h_res, h_args = funcs[name]
        have = set_.get(name, {})
        if 'restype' in have:
            if kind(have['restype']) != h_res:
                said.append('%s: returns %s in the header, %s in the example' % (name, h_res, kind(have['restype'])))
        elif name in called and h_res != 'i4':
            said.append('%s: called without a restype, but returns %s in the header' % (name, h_res))
        if 'argtypes' in have:
            got = [kind(a) for a in have['argtypes']]
            if len(got) != len(h_args):
                said.append('%s: %d arguments in the header, %d in the example' % (name, len(h_args), len(got)))
            said += ['%s: argument %d is %s in the header, %s in the example' % (name, j, h, g)
                     for j, (g, h) in enumerate(zip(got, h_args)) if g != h]
    return said, set_, called


def test_the_example_binding_agrees_with_the_header(tmp_path, monkeypatch):
    said, set_, called = compare_example(os.path.join(ROOT, 'examples', 'ndcn_hip_binding.py'), tmp_path, monkeypatch)
    assert said == []
    assert 'ndcn_rhs_f32' in set_ and 'argtypes' in set_['ndcn_rhs_f32'] and 'ndcn_rhs_f32' in called     # the recorder saw the file
