"""One-off: are the gfx950 kernels of two builds of a library the same?  Usage:
    python compare_device_code.py PARENT.so NEW.so [PARENT.so NEW.so ...]
Extracts the gfx950 code objects of each .so (llvm-objdump --offloading), disassembles them (llvm-objdump -d) and compares
per symbol: code addresses are dropped, instruction text and encodings kept.  A diff of two disassemblies, nothing else."""
import os
import re
import shutil
import subprocess
import sys
import tempfile

OBJDUMP = os.environ.get('LLVM_OBJDUMP', '/opt/rocm/llvm/bin/llvm-objdump')


def kernels(so):
    """-> (number of code objects that hold code, {symbol: [instruction text + encoding, ...]})"""
    work = tempfile.mkdtemp()
    try:
        shutil.copy(so, os.path.join(work, 'lib.so'))
        subprocess.run([OBJDUMP, '--offloading', 'lib.so'], cwd=work, check=True, capture_output=True)
        symbols, objects = {}, 0
        for name in sorted(os.listdir(work)):
            if 'gfx950' not in name:
                continue
            text = subprocess.run([OBJDUMP, '-d', name], cwd=work, check=True, capture_output=True, text=True).stdout
            current = None
            for line in text.splitlines():
                m = re.match(r'^[0-9a-f]+ <(.+)>:$', line)
                if m:
                    current = symbols.setdefault(m.group(1), [])
                elif current is not None and line.startswith('\t'):
                    current.append(re.sub(r'//\s*[0-9A-Fa-f]+:', '//', line).strip())
            objects += current is not None
        return objects, symbols
    finally:
        shutil.rmtree(work)


def main(paths):
    worst = 0
    for parent, new in zip(paths[0::2], paths[1::2]):
        (po, ps), (no, ns) = kernels(parent), kernels(new)
        differ = sorted(s for s in set(ps) & set(ns) if ps[s] != ns[s])
        print(os.path.basename(new))
        print(f'  code objects with kernels: {po} and {no}')
        print(f'  symbols: {len(ps)} and {len(ns)}, {"the same names" if set(ps) == set(ns) else "NAMES DIFFER: " + str(sorted(set(ps) ^ set(ns)))}')
        print(f'  instructions: {sum(map(len, ps.values()))} and {sum(map(len, ns.values()))}')
        print(f'  symbols whose instruction text differs: {len(differ)} {differ if differ else ""}')
        worst += len(differ) + (set(ps) != set(ns))
    return 1 if worst else 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]))
