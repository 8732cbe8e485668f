"""device_code_diff.py <git-ref> [file.hip ...]: does a source change leave the gfx950 device code alone?

Compiles the named sources (default: every .hip under cleandiffuser_amd/csrc) to device-only assembly, once from a temporary git worktree
of <git-ref> and once from the working tree, with the flags build() uses, and compares the text per function symbol: comments and
.loc/.file/.ident/.p2align dropped, local labels renumbered in order of appearance.  Prints SAME / DIFF / ONLY-IN per symbol and exits
non-zero on any difference.  Needs no GPU; each run costs two full compiles."""
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import __graft_entry__ as ge  # noqa: E402

REL = os.path.relpath(ge.CSRC, ge.ROOT)


def compile_asm(job):
    root, name, out = job
    subprocess.run([ge.HIPCC, *ge.FLAGS, "-I", os.path.join(root, "include"), *ge.EXTRA_FLAGS.get(name, []),
                    "--cuda-device-only", "-S", os.path.join(root, REL, name), "-o", out], check=True)


def functions(path):
    """{symbol: normalised body} of one assembly file: the lines from 'sym:' to its .size, plus a kernel's .amdhsa_kernel block
    (register counts, LDS bytes)."""
    out, sym, labels = {}, None, {}
    for line in open(path):
        line = re.sub(r"\s*;.*", "", line).strip()
        if not line or re.match(r"\.(loc|file|ident|p2align)\b", line):
            continue
        m = re.match(r"\.type\s+(\S+),@function$|\.amdhsa_kernel (\S+)$", line)
        if sym is None and m:
            sym, labels = m.group(1) or m.group(2), {}
            out.setdefault(sym, [])
        elif sym is not None:
            line = re.sub(r"\.L(?:BB\d+_|tmp|func_end|func_begin)\d+", lambda t: labels.setdefault(t.group(0), f".L{len(labels)}"), line)
            out[sym].append(line)
            if line.startswith((".size", ".end_amdhsa_kernel")):
                sym = None
    return out


def main(ref, names):
    names = names or sorted(f for f in os.listdir(ge.CSRC) if f.endswith(".hip"))
    names = [os.path.basename(n) for n in names]
    bad = total = 0
    with tempfile.TemporaryDirectory() as tmp:
        tree = os.path.join(tmp, "tree")
        subprocess.run(["git", "-C", ge.ROOT, "worktree", "add", "--detach", tree, ref], check=True, stdout=subprocess.DEVNULL)
        try:
            jobs = [(root, n, os.path.join(tmp, f"{tag}_{n}.s")) for n in names for tag, root in (("old", tree), ("new", ge.ROOT))]
            with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex:
                list(ex.map(compile_asm, jobs))
        finally:
            subprocess.run(["git", "-C", ge.ROOT, "worktree", "remove", "--force", tree], check=True)
        for n in names:
            old, new = (functions(os.path.join(tmp, f"{tag}_{n}.s")) for tag in ("old", "new"))
            for sym in sorted(set(old) | set(new)):
                verdict = "SAME" if old.get(sym) == new.get(sym) else "DIFF" if sym in old and sym in new else \
                    f"ONLY-IN-{'OLD' if sym in old else 'NEW'}"
                bad, total = bad + (verdict != "SAME"), total + 1
                print(f"{verdict:12s} {n}  {sym}")
    print(f"{total} symbols, {bad} difference(s)")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2:]))
