"""Register / scratch audit of the device code inside a built library: every kernel's VGPR / SGPR counts, spills and
private-segment (scratch) bytes from the code objects' AMDGPU metadata notes.
Usage: python tools/check_codeobj.py [simgan_amd/libsimgan_hip.so]      (needs /opt/rocm/lib/llvm/bin; no GPU)
Prints one line per kernel that spills VGPRs or uses scratch memory and a summary; exit status 1 if any does.
       python tools/check_codeobj.py --diff OLD.so NEW.so
Compares two builds kernel by kernel: the code bytes (the symbol's address and size in .text) and the metadata (registers,
spills, scratch, LDS, kernarg segment size).  Prints the kernels present on one side only and those that differ, with a size
table; exit status 1 if anything differs.  A byte comparison: what a refactor that claims "same code" has to show."""
import os
import re
import struct
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def code_objects(lib):
    """-> list of gfx code-object byte strings inside the library's .hip_fatbin section."""
    with tempfile.TemporaryDirectory() as td:
        fat = os.path.join(td, "fat.bin")
        subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", f".hip_fatbin={fat}", lib, os.path.join(td, "x")], check=True)
        data = open(fat, "rb").read()
    out = []
    for m in re.finditer(MAGIC, data):
        base = m.start()
        (n,) = struct.unpack_from("<Q", data, base + len(MAGIC))
        off = base + len(MAGIC) + 8
        for _ in range(n):
            o, sz, tl = struct.unpack_from("<QQQ", data, off)
            triple = data[off + 24:off + 24 + tl].decode()
            off += 24 + tl
            if "amdgcn" in triple and sz:
                out.append(data[base + o:base + o + sz])
    return out


def function_bytes(co):
    """-> {name: code bytes} for every function symbol of an ELF64 code object that lies in .text."""
    shoff, = struct.unpack_from("<Q", co, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", co, 0x3A)
    secs = [struct.unpack_from("<IIQQQQIIQQ", co, shoff + i * shentsize) for i in range(shnum)]   # name type flags addr offset size link info align entsize
    cstr = lambda tab, o: co[tab[4] + o:co.index(b"\0", tab[4] + o)].decode()  # noqa: E731
    text = next(i for i, sec in enumerate(secs) if cstr(secs[shstrndx], sec[0]) == ".text")
    out = {}
    for sec in secs:
        if sec[1] != 2:   # SHT_SYMTAB
            continue
        for o in range(sec[4], sec[4] + sec[5], 24):
            name, info, _, shndx, value, size = struct.unpack_from("<IBBHQQ", co, o)
            if (info & 15) == 2 and shndx == text and size:   # STT_FUNC
                start = secs[text][4] + value - secs[text][3]
                out[cstr(secs[sec[6]], name)] = co[start:start + size]
    return out


def kernels(lib):
    res = []
    for co in code_objects(lib):
        code = function_bytes(co)
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(co)
            f.flush()
            txt = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", f.name], capture_output=True, text=True).stdout
        for blk in re.split(r"\n\s*- \.agpr_count:", txt)[1:]:
            g = lambda key: (re.search(rf"\.{key}:\s*(\S+)", blk) or [None, "0"])[1]  # noqa: E731
            res.append({"name": g("name"), "vgpr": int(g("vgpr_count")), "sgpr": int(g("sgpr_count")), "vgpr_spill": int(g("vgpr_spill_count")),
                        "sgpr_spill": int(g("sgpr_spill_count")), "scratch": int(g("private_segment_fixed_size")), "lds": int(g("group_segment_fixed_size")),
                        "kernarg": int(g("kernarg_segment_size")), "code": code[g("name")]})
    return res


META = ("vgpr", "sgpr", "vgpr_spill", "sgpr_spill", "scratch", "lds", "kernarg")


def diff(old_lib, new_lib):
    """Prints what differs between the kernels of two libraries; -> number of kernels that are not identical."""
    def by_name(lib):   # a kernel that several translation units instantiate appears once per code object: name, name #2, ...
        out, seen = {}, {}
        for k in kernels(lib):
            seen[k["name"]] = seen.get(k["name"], 0) + 1
            out[k["name"] + (f" #{seen[k['name']]}" if seen[k["name"]] > 1 else "")] = k
        return out, len(seen)
    (old, old_names), (new, new_names) = by_name(old_lib), by_name(new_lib)
    for side, a, b in (("old", old, new), ("new", new, old)):
        for name in sorted(set(a) - set(b)):
            print(f"only in {side}: {name} ({len(a[name]['code'])} B)")
    changed = 0
    for name in sorted(set(old) & set(new)):
        o, n = old[name], new[name]
        what = [f"{key} {o[key]} -> {n[key]}" for key in META if o[key] != n[key]]
        if len(o["code"]) != len(n["code"]):
            what.append(f"code size {len(o['code'])} -> {len(n['code'])} B")
        elif o["code"] != n["code"]:
            what.append(f"{sum(x != y for x, y in zip(o['code'], n['code']))} of {len(o['code'])} code bytes differ")
        if what:
            changed += 1
            print(f"differs: {name}: " + "; ".join(what))
    both = len(set(old) & set(new))
    print(f"{len(old)} kernels ({old_names} names) in {old_lib}, {len(new)} ({new_names}) in {new_lib}: {both - changed} identical (code bytes and metadata), {changed} differ, "
          f"{len(set(old) ^ set(new))} on one side only")
    return changed + len(set(old) ^ set(new))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--diff":
        sys.exit(1 if diff(sys.argv[2], sys.argv[3]) else 0)
    lib = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "simgan_amd", "libsimgan_hip.so")
    ks = kernels(lib)
    bad = [k for k in ks if k["vgpr_spill"] or k["scratch"]]     # (SGPR spills go to VGPR lanes, not to memory: reported, not failed)
    for k in bad:
        print(f"{k['name']}: {k['vgpr_spill']} VGPR / {k['sgpr_spill']} SGPR spills, {k['scratch']} B scratch")
    print(f"{len(ks)} kernels in {lib}: {len(bad)} with VGPR spills or scratch; {sum(1 for k in ks if k['sgpr_spill'])} spill SGPRs into VGPR lanes "
          f"(max {max(k['sgpr_spill'] for k in ks)}); max VGPRs {max(k['vgpr'] for k in ks)}")
    sys.exit(1 if bad else 0)
