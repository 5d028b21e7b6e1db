"""Which compiled kernel instances libmlbp.so holds, and which of them a call launched.

A kernel's host-side handle -- the address the library launches it by, and what mlbp_launch_log records -- is a local data
symbol of the .so named with the kernel's mangled name.  This module reads the ELF .symtab with `struct` alone (no nm or
c++filt needed), decodes the template arguments the sweep and contraction kernels use (`Li<n>E`, `Lb0E` / `Lb1E`, `d`, `f`)
and maps launch-log handles back to instances such as ('sweep_x64_lean_kernel', (3, False, False, 0, True)).

compiled() / launched() see the instances of FAMILIES only; all_compiled() / all_launched() see every kernel of the library,
a plain one as (name, ()).  kernel_names() reads the names of the __global__ functions from the HIP sources, to check the
symbol reader against.
"""
import glob
import os
import ctypes as C
import re
import struct

from macaronicusermodeling_amd import _ffi

# The templated sweep and contraction families: tests/test_kernel_inventory.py requires every compiled instance of these to
# be COVERED by a GPU parity case or UNREACHABLE with a reason.
FAMILIES = ('sweep_x64_shared_kernel', 'sweep_x64_lean_kernel', 'sweep_wide_kernel', 'contract_kernel',
            'sweep_x64_fused_kernel', 'sweep_generic_kernel', 'contract_chunked_kernel', 'gradient_kernel',
            'gradient_x64_kernel', 'shared_prepare_kernel', 'table_frag_kernel')

_SHT_SYMTAB = 2
_STT_OBJECT, _STT_FUNC = 1, 2


def _symbols(path):
    """{name: (st_value, st_type)} of the ELF64 little-endian file's .symtab."""
    data = open(path, 'rb').read()
    if data[:4] != b'\x7fELF' or data[4] != 2 or data[5] != 1:
        raise ValueError('%s is not a little-endian ELF64 file' % path)
    e_shoff, = struct.unpack_from('<Q', data, 0x28)
    e_shentsize, e_shnum = struct.unpack_from('<HH', data, 0x3A)
    sections = [struct.unpack_from('<IIQQQQIIQQ', data, e_shoff + i * e_shentsize) for i in range(e_shnum)]
    out = {}
    for sh in sections:
        if sh[1] != _SHT_SYMTAB:
            continue
        off, size, link, entsize = sh[4], sh[5], sh[6], sh[9]
        stroff = sections[link][4]
        for k in range(size // entsize):
            st_name, st_info, _, _, st_value, _ = struct.unpack_from('<IBBHQQ', data, off + k * entsize)
            if not st_name:
                continue
            end = data.index(b'\0', stroff + st_name)
            out[data[stroff + st_name:end].decode()] = (st_value, st_info & 0xF)
    if not out:
        raise ValueError('%s has no .symtab (stripped?)' % path)
    return out


_ARG = re.compile(r'Li(n?)(\d+)E|Lb([01])E|([df])')


def decode(mangled):
    """('family', (template args...)) for a mangled kernel symbol of one of FAMILIES, else None."""
    for fam in FAMILIES:
        tag = '%d%sI' % (len(fam), fam)
        i = mangled.find(tag)
        if i < 0:
            continue
        i += len(tag)
        args = []
        while mangled[i] != 'E':
            m = _ARG.match(mangled, i)
            if not m:
                raise ValueError('cannot decode template argument at %r of %s' % (mangled[i:i + 12], mangled))
            if m.group(2) is not None:
                args.append(-int(m.group(2)) if m.group(1) else int(m.group(2)))
            elif m.group(3) is not None:
                args.append(m.group(3) == '1')
            else:
                args.append({'d': 'double', 'f': 'float'}[m.group(4)])
            i = m.end()
        return fam, tuple(args)
    return None


def decode_kernel(mangled):
    """('name', (template args...)) for any mangled kernel symbol -- ('name', ()) for a plain kernel -- else None.  A kernel's
    identifier ends in '_kernel'.  decode(m) == decode_kernel(m) for the instances of FAMILIES.

    The symbol is a name (_Z <len><id>) or a nested one (_ZN <len><id>... E) ending in the kernel's identifier, its template
    arguments if any, then the parameter types: a data symbol without parameter types is a variable, not a kernel."""
    if not mangled.startswith('_Z'):
        return None
    nested = mangled.startswith('_ZN')
    i, ident = 3 if nested else 2, None
    while i < len(mangled) and mangled[i].isdigit():
        j = i
        while mangled[j].isdigit():
            j += 1
        n = int(mangled[i:j])
        ident, i = mangled[j:j + n], j + n
        if not nested:
            break
    if ident is None or not ident.endswith('_kernel') or i >= len(mangled):
        return None
    args = []
    if mangled[i] == 'I':
        i += 1
        while mangled[i] != 'E':
            m = _ARG.match(mangled, i)
            if not m:
                raise ValueError('cannot decode template argument at %r of %s' % (mangled[i:i + 12], mangled))
            if m.group(2) is not None:
                args.append(-int(m.group(2)) if m.group(1) else int(m.group(2)))
            elif m.group(3) is not None:
                args.append(m.group(3) == '1')
            else:
                args.append({'d': 'double', 'f': 'float'}[m.group(4)])
            i = m.end()
        i += 1
    if nested:                                    # the nested name closes
        if mangled[i:i + 1] != 'E':
            return None
        i += 1
    if i >= len(mangled):                         # no parameter types: a variable
        return None
    return ident, tuple(args)


def kernels_of(path):
    """Every kernel instance the shared object at `path` holds, as decode_kernel names them."""
    found = {decode_kernel(n) for n, (_, typ) in _symbols(path).items() if typ == _STT_OBJECT}
    return found - {None}


def exported_functions(path):
    """The sorted names of the mlbp_* functions the shared object at `path` exports."""
    return sorted(n for n, (_, typ) in _symbols(path).items() if n.startswith('mlbp_') and typ == _STT_FUNC)


_cache = {}


def _tables():
    if not _cache:
        syms = _symbols(_ffi.LIB_PATH)
        fn = _ffi.lib.mlbp_last_sweep_kernel
        base = C.cast(fn, C.c_void_p).value - syms['mlbp_last_sweep_kernel'][0]
        by_addr, instances, all_by_addr = {}, set(), {}
        for name, (value, typ) in syms.items():
            if typ != _STT_OBJECT:
                continue
            kern = decode_kernel(name)
            if kern is not None:
                all_by_addr[base + value] = kern
            inst = decode(name)
            if inst is None:
                continue
            instances.add(inst)
            by_addr[base + value] = inst
        _cache['instances'] = frozenset(instances)
        _cache['by_addr'] = by_addr
        _cache['all'] = frozenset(all_by_addr.values())
        _cache['all_by_addr'] = all_by_addr
    return _cache


def compiled():
    """Every instance of FAMILIES that libmlbp.so holds."""
    return _tables()['instances']


def reset():
    _ffi.lib.mlbp_launch_log_reset()


def launched_handles():
    n = _ffi.lib.mlbp_launch_log(None, 0)
    buf = (C.c_void_p * max(n, 1))()
    n = min(n, _ffi.lib.mlbp_launch_log(buf, len(buf)))
    return [buf[i] for i in range(n)]


def launched():
    """The instances of FAMILIES in the calling thread's launch log since reset(), in launch order."""
    by_addr = _tables()['by_addr']
    return [by_addr[h] for h in launched_handles() if h in by_addr]


def all_compiled():
    """Every kernel libmlbp.so holds: each instance of a templated kernel as (name, args), a plain kernel as (name, ())."""
    return _tables()['all']


def all_launched():
    """Every kernel in the calling thread's launch log since reset(), in launch order, as all_compiled() names it."""
    by_addr = _tables()['all_by_addr']
    return [by_addr[h] for h in launched_handles() if h in by_addr]


CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'macaronicusermodeling_amd', 'csrc')
_COMMENT = re.compile(r'//[^\n]*|/\*.*?\*/', re.S)
_GLOBAL = re.compile(r'__global__[^;{]*?\bvoid\s+(\w+)\s*\(')


def kernel_names(csrc=CSRC):
    """The names of the __global__ functions defined in the library's HIP sources (comments stripped)."""
    names = set()
    for path in sorted(glob.glob(os.path.join(csrc, '*.hip')) + glob.glob(os.path.join(csrc, '*.h'))):
        names.update(_GLOBAL.findall(_COMMENT.sub('', open(path).read())))
    return names
