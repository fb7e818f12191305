"""What the three ABI tests (test_abi, test_gallery_abi, test_gallery_text_abi) share: the prototypes a C header declares and the symbols a
built library exports."""
import re
import subprocess


def _prototypes(path, prefix):
    """{entry point: number of arguments} of the `int` / `const char*` prototypes named <prefix>... in the header at path"""
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    protos = {}
    for m in re.finditer(r"(?:int|const char\*)\s*(%s\w+)\s*\(([^;]*?)\)\s*;" % prefix, text, flags=re.S):
        args = m.group(2).strip()
        protos[m.group(1)] = 0 if args in ("", "void") else len([a for a in args.split(",") if a.strip()])
    return protos


def _exported(lib_path):
    """the dynamic symbols a library defines (`nm -D`), without the linker's and the HIP runtime's own"""
    out = subprocess.run(["nm", "-D", "--defined-only", lib_path], stdout=subprocess.PIPE, text=True, check=True).stdout
    syms = {l.split()[-1] for l in out.splitlines() if l.strip()}
    return {s for s in syms if not s.startswith(("__hip", "_init", "_fini", "__bss", "_edata", "_end"))}
