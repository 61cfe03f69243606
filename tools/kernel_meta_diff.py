"""Compare the gfx950 device code of two builds, kernel by kernel.

  python tools/kernel_meta_diff.py OLD NEW     (two objects / libraries, or two build directories of *.o)

For every offload bundle in the files it compares, per kernel, the register / spill / LDS metadata and the code itself:
the bytes of every FUNC symbol and of every *.kd kernel descriptor (bytes 16..23 masked: the code-entry offset, which
moves when kernels reorder). __hip_cuid_* is ignored. One summary line per file; exit status 1 when a symbol present in
both builds differs or a symbol is new (removed ones are listed: a refactor that drops kernels expects them).
"""
import os
import re
import struct
import subprocess
import sys
import tempfile

READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def code_objects(path):
    """the gfx950 ELF images of every offload bundle in a file"""
    data = open(path, "rb").read()
    for m in re.finditer(MAGIC, data):
        off = m.start()
        n = int.from_bytes(data[off + 24:off + 32], "little")
        p = off + 32
        for _ in range(n):
            eoff, esz, tl = struct.unpack_from("<QQQ", data, p)
            triple = data[p + 24:p + 24 + tl].decode()
            p += 24 + tl
            if "gfx950" in triple:
                yield data[off + eoff:off + eoff + esz]


def metadata(blob):
    """kernel name -> (vgprs, spilled vgprs, static LDS bytes) from the code object's notes"""
    with tempfile.NamedTemporaryFile(suffix=".co") as f:
        f.write(blob)
        f.flush()
        out = subprocess.run([READELF, "--notes", f.name], capture_output=True, text=True).stdout
    res = {}
    for blk in out.split("  - .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk)
        vals = [re.search(r"\.%s:\s+(\d+)" % k, blk) for k in ("vgpr_count", "vgpr_spill_count", "group_segment_fixed_size")]
        if name:
            res[name.group(1)] = tuple(v and int(v.group(1)) for v in vals)
    return res


def symbols(blob):
    """symbol name -> bytes, for the functions and kernel descriptors of an ELF64 code object"""
    shoff, = struct.unpack_from("<Q", blob, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", blob, 0x3A)
    secs = [struct.unpack_from("<IIQQQQIIQQ", blob, shoff + i * shentsize) for i in range(shnum)]
    res = {}
    for sec in secs:
        if sec[1] != 2:  # SHT_SYMTAB
            continue
        stroff = secs[sec[6]][4]
        for i in range(sec[5] // 24):
            name, info, _, shndx, value, size = struct.unpack_from("<IBBHQQ", blob, sec[4] + 24 * i)
            end = blob.index(b"\0", stroff + name)
            sym = blob[stroff + name:end].decode()
            kd = sym.endswith(".kd")
            if not size or shndx == 0 or shndx >= shnum or sym.startswith("__hip_cuid_") or not (info & 15 == 2 or kd):
                continue
            s = secs[shndx]
            raw = bytearray(blob[s[4] + value - s[3]:s[4] + value - s[3] + size])
            if kd:
                raw[16:24] = bytes(8)
            res[sym] = bytes(raw)
    return res


def collect(path):
    meta, syms = {}, {}
    if not os.path.exists(path):  # a translation unit that only one of the two builds has
        return meta, syms
    for blob in code_objects(path):
        meta.update(metadata(blob))
        syms.update(symbols(blob))
    return meta, syms


def compare(old, new, label):
    (ma, sa), (mb, sb) = collect(old), collect(new)
    changed = sorted(k for k in set(sa) & set(sb) if sa[k] != sb[k])
    meta = sorted(k for k in set(ma) & set(mb) if ma[k] != mb[k])
    removed, added = sorted(set(sa) - set(sb)), sorted(set(sb) - set(sa))
    nk = lambda names: sum(1 for k in names if k.endswith(".kd"))
    print(f"{label}: {nk(sa)} -> {nk(sb)} kernels, {len(set(sa) & set(sb))} common symbols: {len(changed)} changed, "
          f"{len(meta)} with other metadata, {nk(removed)} kernels removed, {len(added)} symbols new")
    for tag, names in (("changed", changed), ("metadata", meta), ("removed", removed), ("new", added)):
        for k in names:
            if not (tag == "removed" and k.endswith(".kd")):
                print(f"  {tag}: {k[:150]}" + (f" {ma[k]} -> {mb[k]}" if tag == "metadata" else ""))
    return not (changed or meta or added)


if __name__ == "__main__":
    old, new = sys.argv[1:3]
    if os.path.isdir(old):
        names = sorted(set(f for d in (old, new) for f in os.listdir(d) if f.endswith(".o")))
        ok = all([compare(os.path.join(old, f), os.path.join(new, f), f) for f in names])
    else:
        ok = compare(old, new, os.path.basename(new))
    sys.exit(0 if ok else 1)
