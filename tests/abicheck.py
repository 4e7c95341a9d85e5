"""What the host tests ask of the built library and of the C++ header with nm and g++: one definition each. The
tests keep their own skip conditions (shutil.which), symbol tuples, sources and assertions."""
import pathlib
import subprocess

REPO = pathlib.Path(__file__).resolve().parent.parent


def _names(*nm_args):
    out = subprocess.run(["nm", *nm_args], capture_output=True, text=True, check=True).stdout
    return {l.split()[-1] for l in out.splitlines() if l.strip()}


def defined_symbols(lib_path):
    """The dynamic symbols a shared library defines."""
    return _names("-D", "--defined-only", str(lib_path))


def undefined_symbols(obj):
    """The symbols an object file needs from elsewhere."""
    return _names("-u", str(obj))


def compile_class_user(tmp_path, stem, source):
    """`source` as tmp_path/stem.cpp, compiled as an application that includes Sphereflake.hpp would compile it; the
    object file."""
    src, obj = tmp_path / f"{stem}.cpp", tmp_path / f"{stem}.o"
    src.write_text(source)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-c", f"-I{REPO / 'include'}",
                        f"-I{REPO / 'sphereflake-raytracer_amd' / 'csrc'}", str(src), "-o", str(obj)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return obj
