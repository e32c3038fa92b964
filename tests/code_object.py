"""What the compiler says about the kernels of the built library: the ONE reader of the gfx950 code object inside liblfi_hip.so, for the tests
and for tools/ (which put tests/ on sys.path).  Every function takes the library's path (native.build.HIP_LIB).

    path(lib)      the gfx950 ELF, cut out of the clang offload bundle once per (library, mtime, size)
    kernels(lib)   {mangled name: record}: the scalar fields of each entry of amdhsa.kernels (llvm-readelf --notes, run once)
    bodies(lib)    {symbol: disassembly text} (llvm-objdump -d, run once)
    named(d, stem) the entries of either whose symbol is exactly lfi::<stem>, plain or templated
"""
import atexit
import functools
import os
import re
import shutil
import struct
import subprocess
import tempfile


def tool(name):
    """An LLVM tool of the ROCm installation whose hipcc built the library: beside the compiler's own"""
    hipcc = shutil.which(os.environ.get("HIPCC", "hipcc")) or "/opt/rocm/bin/hipcc"
    roots = [os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), os.environ.get("ROCM_PATH", "/opt/rocm"), "/opt/rocm"]
    for root in roots:
        for sub in ("lib/llvm/bin", "llvm/bin"):
            found = os.path.join(root, sub, name)
            if os.path.exists(found):
                return found
    raise AssertionError(f"{name} not found under {roots}: the library was built with ROCm's hipcc, its LLVM tools belong to the same installation")


def have_tools():
    try:
        return bool(tool("llvm-readelf") and tool("llvm-objdump"))
    except AssertionError:
        return False


def path(lib):
    st = os.stat(lib)
    return _extract(os.path.abspath(lib), st.st_mtime_ns, st.st_size)


@functools.lru_cache(maxsize=None)
def _extract(lib, mtime, size):
    data = open(lib, "rb").read()
    i = data.find(b"__CLANG_OFFLOAD_BUNDLE__")
    assert i >= 0, f"{lib} holds no clang offload bundle"
    # header: magic (24 bytes), number of entries; per entry: offset, size, length of the target triple, the triple
    n = struct.unpack_from("<Q", data, i + 24)[0]
    off = i + 32
    for _ in range(n):
        o, sz, tl = struct.unpack_from("<QQQ", data, off)
        off += 24
        triple = data[off:off + tl]
        off += tl
        if b"gfx950" in triple:
            tmp = tempfile.mkdtemp(prefix="lfi_code_object_")
            atexit.register(shutil.rmtree, tmp, ignore_errors=True)
            co = os.path.join(tmp, "gfx950.co")
            with open(co, "wb") as f:
                f.write(data[i + o:i + o + sz])
            return co
    raise AssertionError("no gfx950 code object in the bundle")


@functools.lru_cache(maxsize=None)
def _run(name, *args):
    return subprocess.run([tool(name), *args], capture_output=True, text=True, check=True).stdout


def notes(lib):
    """the text of llvm-readelf --notes: the code object's metadata as a YAML document"""
    return _run("llvm-readelf", "--notes", path(lib))


def _scalar(text):
    if re.fullmatch(r"-?\d+", text):
        return int(text)
    if text in ("true", "false"):
        return text == "true"
    return text[1:-1] if len(text) >= 2 and text[0] == text[-1] and text[0] in "'\"" else text


def parse_notes(text):
    """{.name: record} of amdhsa.kernels.  An entry begins at its list item ("  - .key: value") and ends at the next one; its own keys stand
    four columns in, sorted — so .agpr_count and .group_segment_fixed_size come BEFORE the .name they belong to.  Deeper lines (the entries
    of .args, the items of .language_version) and keys without a value of their own (.args:) are not scalar fields and are skipped."""
    lines = text.splitlines()
    records, cur = [], None
    for line in lines[lines.index("amdhsa.kernels:") + 1:]:
        if line[:1] not in (" ", ""):       # the next top-level key: amdhsa.target
            break
        if line.startswith("  - "):
            cur = {}
            records.append(cur)
            line = "    " + line[4:]
        m = re.fullmatch(r"    (\.\w+):\s+(\S.*)", line)
        if m:
            cur[m.group(1)] = _scalar(m.group(2).rstrip())
    assert all(".name" in r for r in records) and len({r[".name"] for r in records}) == len(records)
    return {r[".name"]: r for r in records}


def kernels(lib):
    return _kernels(path(lib))


@functools.lru_cache(maxsize=None)
def _kernels(co):
    return parse_notes(_run("llvm-readelf", "--notes", co))


def bodies(lib):
    return _bodies(path(lib))


@functools.lru_cache(maxsize=None)
def _bodies(co):
    found, cur = {}, None
    for line in _run("llvm-objdump", "-d", co).splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:$", line)
        if m:
            cur = found.setdefault(m.group(1), [])
        elif cur is not None:
            cur.append(line)
    return {k: "\n".join(v).rstrip("\n") for k, v in found.items()}


def named(records, stem):
    """the entries of kernels() or bodies() that ARE lfi::<stem>: _ZN3lfi<len><stem> followed by I (template arguments) or E (none), so that
    yuvs_expand never picks up a yuvs_expand_something, nor yuvs_derived_expand by a careless substring"""
    prefix = f"_ZN3lfi{len(stem)}{stem}"
    return {k: v for k, v in records.items() if k.startswith(prefix) and k[len(prefix):len(prefix) + 1] in ("I", "E")}
