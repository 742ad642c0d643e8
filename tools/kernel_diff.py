"""Compare the gfx950 kernels of two builds, per kernel: the bytes of each kernel function and of its kernel descriptor
(<name>.kd: VGPRs, SGPRs, LDS, scratch).  Prints the number of kernels on each side, the symbols only one side has,
the symbols whose bytes differ, and one sha256 over the sorted per-kernel hashes.  An input is a libdsx.so, an offload
bundle (hipcc --offload-device-only -c) or a bare code object; the kernels of every gfx950 code object in it are taken
together.  The descriptor's offset to its function (bytes 16..23) depends on the order of the kernels in the file and is
left out of the comparison.

    python tools/kernel_diff.py A B [REGEX]        (REGEX: only kernels whose mangled name matches, e.g. k_conv)"""
import hashlib, re, struct, sys

BUNDLE = b"__CLANG_OFFLOAD_BUNDLE__"


def code_objects(blob):
    """the gfx950 ELF code objects inside a shared library / bundle / code object"""
    if blob[:4] == b"\x7fELF" and struct.unpack_from("<H", blob, 18)[0] == 224:   # EM_AMDGPU
        return [blob]
    out, at = [], blob.find(BUNDLE)
    while at >= 0:
        (n,) = struct.unpack_from("<Q", blob, at + 24)
        p = at + 32
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", blob, p)
            triple = blob[p + 24:p + 24 + tlen].decode()
            p += 24 + tlen
            if "gfx950" in triple: out.append(blob[at + off:at + off + size])
        at = blob.find(BUNDLE, at + 24)
    assert out, "no gfx950 code object found (compressed bundles are not read)"
    return out


def kernels(elf):
    """{name: (function bytes, descriptor bytes)} of one code object"""
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", elf, 0x3A)
    sec = [struct.unpack_from("<IIQQQQIIQQ", elf, shoff + i * shentsize) for i in range(shnum)]
    symtab = next(s for s in sec if s[1] == 2)
    strtab = sec[symtab[6]]
    sym = {}
    for o in range(symtab[4], symtab[4] + symtab[5], 24):
        name, info, _, shndx, value, size = struct.unpack_from("<IBBHQQ", elf, o)
        if size == 0 or shndx == 0 or shndx >= shnum: continue
        s = strtab[4] + name
        nm = elf[s:elf.index(b"\0", s)].decode()
        at = sec[shndx][4] + value - sec[shndx][3]
        sym[nm] = (info & 15, elf[at:at + size])
    out = {}
    for nm, (typ, data) in sym.items():
        if nm.endswith(".kd") and nm[:-3] in sym:
            out[nm[:-3]] = (sym[nm[:-3]][1], data[:16] + bytes(8) + data[24:])
    return out


def load(path, pat):
    ks = {}
    for elf in code_objects(open(path, "rb").read()):
        for nm, v in kernels(elf).items():
            if pat.search(nm):
                assert nm not in ks, nm
                ks[nm] = v
    return ks


a_path, b_path = sys.argv[1:3]
pat = re.compile(sys.argv[3] if len(sys.argv) > 3 else "")
A, B = load(a_path, pat), load(b_path, pat)
for tag, ks in (("A", A), ("B", B)):
    h = hashlib.sha256()
    for nm in sorted(ks): h.update(hashlib.sha256(nm.encode() + b"\0" + ks[nm][0] + ks[nm][1]).digest())
    print(f"{tag}: {len(ks)} kernels  sha256 {h.hexdigest()}")
for nm in sorted(set(A) - set(B)): print("only in A:", nm)
for nm in sorted(set(B) - set(A)): print("only in B:", nm)
diff = [nm for nm in sorted(set(A) & set(B)) if A[nm] != B[nm]]
for nm in diff:
    print("differs:", nm, "function" if A[nm][0] != B[nm][0] else "", "descriptor" if A[nm][1] != B[nm][1] else "")
common = hashlib.sha256()
for nm in sorted(set(A) & set(B)): common.update(hashlib.sha256(nm.encode() + b"\0" + A[nm][0] + A[nm][1]).digest())
print(f"common: {len(set(A) & set(B))} kernels, {len(diff)} differ" + ("" if diff else f"  sha256 {common.hexdigest()}"))
sys.exit(1 if diff else 0)
