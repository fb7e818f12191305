"""What the ABI tests (test_abi, test_<side library>_abi) share: the prototypes a C header declares, the symbols a built library exports
and the resource reports of the other libraries."""
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


def _other_reports(name):
    """the resource reports of the product library and of every side library but `name`"""
    from clip_fsar_amd import build as b
    others = [b.USAGE] + [b.SIDE_LIBS[n].usage for n in b.side_lib_names() if n != name]
    assert len(others) == 6 and b.SIDE_LIBS[name].usage not in others
    return others
