"""Per-kernel identity of two gfx950 assembly listings of marlnav_step.hip
(`make asm` output, or the same compile of another revision): for every
kernel of the first listing whose name matches PATTERN, the sha256 of its
code (label to .Lfunc_end) in both listings, after the differences that are
not code are normalised away: the kernel's own symbol (a template parameter
added with a default changes the mangled name), the translation unit's
function numbering in local labels (.LBB<n>_, .Lfunc_begin/end<n>: kernels
added to the file renumber them), comments (they name basic blocks by that
numbering) and __hip_cuid_ lines. Kernels are matched
by demangled name with the default `(anonymous namespace)::BlockDynamic`
argument dropped.
usage: python scripts/isa_identity_kernels.py parent.s head.s [PATTERN]"""
import hashlib
import re
import subprocess
import sys


def kernels(path):
    out, name, body = {}, None, []
    for line in open(path):
        m = re.match(r"^(_Z\w+):\s", line)
        if name is None and m:
            name, body = m.group(1), []
            continue
        if name is not None:
            if re.match(r"^\.Lfunc_end\d+:", line):
                out[name] = body
                name = None
            else:
                body.append(line)
    return out


def demangle(names):
    txt = subprocess.run(["c++filt"], input="\n".join(names),
                         capture_output=True, text=True, check=True).stdout.split("\n")
    return dict(zip(names, txt))


def norm_name(d):
    return d.replace(", (anonymous namespace)::BlockDynamic>", ">")


def digest(sym, body):
    h = hashlib.sha256()
    n = 0
    for line in body:
        if "__hip_cuid_" in line:
            continue
        line = line.split(";")[0].rstrip() + "\n"  # (comments carry function numbers)
        if not line.strip():
            continue
        line = line.replace(sym, "KERNEL")
        line = re.sub(r"\.LBB\d+_", ".LBB_", line)
        line = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", line)
        h.update(line.encode())
        n += 1
    return h.hexdigest(), n


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    pat = re.compile(sys.argv[3] if len(sys.argv) > 3 else ".")
    da, db = demangle(list(a)), demangle(list(b))
    by_name = {norm_name(d): s for s, d in db.items()}
    same = total = 0
    for sym in sorted(a, key=lambda s: da[s]):
        nm = norm_name(da[sym])
        if not pat.search(nm):
            continue
        total += 1
        ha, na = digest(sym, a[sym])
        other = by_name.get(nm)
        hb, nb = digest(other, b[other]) if other else ("-" * 64, 0)
        same += ha == hb
        print(f"{nm.split('(float')[0].replace('(anonymous namespace)::', '')[5:]:64s} {na:6d} {nb:6d} {ha[:16]} {hb[:16]} "
              f"{'yes' if ha == hb else 'NO'}")
    print(f"# {same} of {total} kernels identical; kernels only in the second listing: "
          f"{len(set(by_name) - {norm_name(d) for d in da.values()})}")
    return 0 if same == total else 1


if __name__ == "__main__":
    sys.exit(main())
