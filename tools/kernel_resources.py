"""VGPR / SGPR / LDS / scratch / code bytes of the kernels in the built library (the code object's metadata notes and symbol table).
usage: kernel_resources.py [library.so] [substring ...]"""
import os, re, subprocess, sys, tempfile
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from settlers_of_catan_rl_amd import _lib
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
t = syms = ""
for co in _lib.device_code_objects(sys.argv[1] if len(sys.argv) > 1 and sys.argv[1].endswith(".so") else None):     # one per translation unit
    with tempfile.NamedTemporaryFile(suffix=".co") as f:
        f.write(co); f.flush()
        t += subprocess.run([READELF, "--notes", f.name], stdout=subprocess.PIPE).stdout.decode()
        syms += subprocess.run([READELF, "-sW", f.name], stdout=subprocess.PIPE).stdout.decode()
code = {}                      # mangled kernel name -> bytes of its function symbol
for line in syms.splitlines():
    p = line.split()
    if len(p) == 8 and p[3] == "FUNC":
        code[p[7]] = p[2]
want = [a for a in sys.argv[1:] if not a.endswith(".so")]
for blk in t.split("  - .agpr_count:")[1:]:
    g = lambda k: (re.search(r"\." + k + r":\s+(\S+)", blk) or [None, "?"])[1]
    name = subprocess.run(["c++filt", g("name")], stdout=subprocess.PIPE).stdout.decode().strip()
    name = re.sub(r"\(.*", "", name)
    if want and not any(w in name for w in want):
        continue
    print(f"{name:70s} vgpr {g('vgpr_count'):>4s} sgpr {g('sgpr_count'):>4s} lds {g('group_segment_fixed_size'):>7s} scratch {g('private_segment_fixed_size'):>5s} wg {g('max_flat_workgroup_size'):>5s} code {code.get(g('name'), '?'):>7s}")
