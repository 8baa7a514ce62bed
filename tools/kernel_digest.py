#!/usr/bin/env python3
"""One line per device function of a translation unit: name, sha256 of its normalised assembly (instructions, the
.amdhsa_* block, its entry in the code-object metadata) and its resource numbers. Two builds ship the same GPU code for
a kernel exactly when its line is the same, whichever unit the kernel lives in:
    python tools/kernel_digest.py deq-mpc-corl_amd/csrc/alqp_quad.hip -DALQP_QUAD_F32 > head.txt
The unit is compiled with the FLAGS of the build.sh next to it, so the same script digests another checkout's sources.
Normalised away: the per-unit function index in local labels (.LBB<i>_<n>, .Lfunc_begin<i>, .Lfunc_end<i>) and the
padding in front of comments."""
import hashlib, os, re, shlex, subprocess, sys, tempfile


def device_asm(src, extra=()):
    """gfx950 assembly of `src`, compiled like build.sh compiles it plus the arguments in `extra`."""
    csrc = os.path.dirname(os.path.abspath(src))
    flags = re.search(r'^FLAGS="(.*)"$', open(os.path.join(csrc, "build.sh")).read(), re.M).group(1)
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "unit.s")
        subprocess.run(["hipcc"] + shlex.split(flags) + ["-S", "--cuda-device-only", os.path.abspath(src), "-o", out] +
                       list(extra), check=True, cwd=csrc, stderr=subprocess.DEVNULL)
        return open(out).read()


def functions(txt):
    """name -> text from the function's label to the end of the resource comments that follow it."""
    lines = txt.split("\n")
    out = {}
    for s in (i for i, l in enumerate(lines) if re.match(r"^\w+:\s+; @", l)):
        name = lines[s].split(":")[0]
        e = next(i for i in range(s, len(lines)) if "; -- End function" in lines[i]) + 1
        while re.match(r"\s*\.set " + re.escape(name) + r"\.|;|\s*\.section\s+\.AMDGPU\.csdata", lines[e]):
            e += 1
        out[name] = "\n".join(lines[s:e])
    return out


def metadata(txt):
    """kernel name -> its entry of amdhsa.kernels."""
    m = re.search(r"amdhsa\.kernels:\n(.*?)\namdhsa\.", txt, re.S)
    out = {}
    for entry in re.split(r"\n(?=  - )", m.group(1) if m else ""):
        name = re.search(r"\.name:\s+(\S+)", entry)
        if name:
            out[name.group(1)] = entry
    return out


def digest(txt):
    meta = metadata(txt)
    rows = []
    for name, body in functions(txt).items():
        body = re.sub(r"(BB|\.Lfunc_begin|\.Lfunc_end)\d+", r"\1#", body)   # BB<i>_<n> also in the loop comments
        body = re.sub(r"[ \t]+;", " ;", body)   # comments are aligned to a column: the padding depends on the label's length
        md = meta.get(name, "")
        num = lambda key, text: (re.search(key + r"\s+(\d+)", text) or [None, "-"])[1]
        rows.append(f"{name} {hashlib.sha256((body + md).encode()).hexdigest()} "
                    f"vgpr={num(r'[.]vgpr_count:', md)} agpr={num(r'[.]agpr_count:', md)} "
                    f"sgpr={num(r'[.]sgpr_count:', md)} scratch={num(r'[.]private_segment_fixed_size:', md)} "
                    f"lds={num(r'[.]group_segment_fixed_size:', md)} occupancy={num(r'; Occupancy:', body)}")
    return sorted(rows)


if __name__ == "__main__":
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    print("\n".join(digest(device_asm(sys.argv[1], sys.argv[2:]))))
