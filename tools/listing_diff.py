#!/usr/bin/env python3
"""Compare two directories of `make -C vulkan-compute-tests_amd asm` output (build/asm: <unit>.s, <unit>.resources.txt) kernel by kernel.

    python tools/listing_diff.py parent/vulkan-compute-tests_amd/build/asm vulkan-compute-tests_amd/build/asm

For every kernel symbol (`.amdhsa_kernel`) of every unit the INSTRUCTION STREAM is compared as text, after this normalisation:
  * assembler directives and blank lines dropped (the kernel descriptor with them), trailing `;` comments dropped;
  * local labels .LBB<n>_<m> renumbered per kernel in the order they first appear (n is the kernel's position in its file);
  * the kernel's own symbol written as <self>; lines naming a __hip_cuid_* object dropped;
  * kernels matched by NAME: the kernel's identifier plus the State types and the integer / bool literals of its template arguments,
    read from the mangled symbol (namespaces and parameter types do not take part, so a kernel may move between namespaces or take
    `typename State::Args`), with the renames of RENAMES applied to the first directory's names.
Where both directories hold <unit>.resources.txt, the figures of -Rpass-analysis=kernel-resource-usage (registers, scratch, LDS,
occupancy, spills) are compared as well.  One line per kernel: `identical`, or the first differing lines.  Exit status 1 on any
difference and on any unit or kernel that only one side has.  It compares text; it looks for no particular instruction."""
import os
import re
import sys

# The per-engine kernels that became instantiations of the mapping templates of csrc/mandel_kernels.h: <engine><mapping>_kernel<U...>
# is <template><State, U...>.  Derived from the engine and mapping names, never from a kernel's content.
ENGINES = {"mandel_perturb": "StatePerturb", "mandel_perturb_deep": "StateDeep"}
MAPPINGS = {"": "mandelbrot_kernel", "_list": "mandelbrot_list_kernel", "_smooth": "mandelbrot_smooth_kernel",
            "_list_smooth": "mandelbrot_list_smooth_kernel", "_block_audit": "mandelbrot_lane_audit_kernel"}
RENAMES = {f"{engine}{mapping}_kernel": (template, state)
           for engine, state in ENGINES.items() for mapping, template in MAPPINGS.items()}
# A BLA unit whose four kernels became one body over a mapping policy: <unit><mapping>_kernel is <unit>_kernel<Map...>.
BLA_UNITS = ("mandel_perturb_bla", "mandel_perturb_bla_deep")
BLA_MAPS = {"": "MapTile", "_list": "MapList", "_smooth": "MapSmoothTile", "_list_smooth": "MapSmoothList"}
RENAMES.update({f"{unit}{mapping}_kernel": (f"{unit}_kernel", policy) for unit in BLA_UNITS for mapping, policy in BLA_MAPS.items()})


def kernel_name(symbol):
    """('mandelbrot_kernel', 'StateF32', 0, 8) for _ZN2mc12_GLOBAL__N_117mandelbrot_kernelINS0_8StateF32ILb0EEELi8EEEvNT_4ArgsE; a symbol
    that is not mangled names itself."""
    if not symbol.startswith("_Z"):
        return (symbol,)
    tokens, i, qualifiers = [], 3 if symbol.startswith("_ZN") else 2, None
    while i < len(symbol):   # the length-prefixed identifiers and the L<type><value>E literals, in order
        lit = re.compile(r"L[a-z](\d+)E").match(symbol, i)
        num = re.compile(r"\d+").match(symbol, i)
        sub = re.compile(r"[ST][0-9A-Z]*_").match(symbol, i)   # a substitution or a template parameter: no identifier
        if lit:
            tokens.append(int(lit.group(1)))
            i = lit.end()
        elif sub and qualifiers is not None:
            i = sub.end()
        elif num:
            n = int(num.group())
            tokens.append(symbol[num.end():num.end() + n])
            i = num.end() + n
        else:
            if qualifiers is None:   # the run of identifiers at the start is the kernel's qualified name
                qualifiers = len(tokens)
            i += 1
    qualifiers = len(tokens) if qualifiers is None else qualifiers
    name = "::".join(t for t in tokens[:qualifiers] if t != "mc" and not t.startswith("_GLOBAL__N"))
    return (name,) + tuple(t for t in tokens[qualifiers:] if isinstance(t, int) or t.startswith(("State", "Map")))


def renamed(name):
    """An old per-engine kernel under its template's name.  (A BLA unit's tile kernel had the name its template has now: a first
    directory that already holds the template, which names its mapping policy, is left as it is.)"""
    if name[0] in RENAMES and not any(isinstance(t, str) and t.startswith("Map") for t in name[1:]):
        template, state = RENAMES[name[0]]
        return (template, state) + name[1:]
    return name


def show(name):
    return name[0] + (f"<{', '.join(str(t) for t in name[1:])}>" if len(name) > 1 else "")


def kernels(text):
    """{kernel name: normalised instruction lines} of one listing."""
    symbols = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M))
    out, symbol, body = {}, None, []
    for line in text.splitlines():
        head = line.split(":")[0]
        if symbol is None:
            if ":" in line and head in symbols:
                symbol, body, labels = head, [], {}
            continue
        if line.startswith(".Lfunc_end"):
            out[kernel_name(symbol)] = body
            symbol = None
            continue
        line = line.split(";")[0].strip()
        if not line or "__hip_cuid_" in line or (line.startswith(".") and not re.match(r"\.LBB\d+_\d+:", line)):
            continue
        line = re.sub(r"\.LBB\d+_\d+", lambda m: labels.setdefault(m.group(), f".LBB_{len(labels)}"), line)
        body.append(re.sub(r"\s+", " ", line.replace(symbol, "<self>")))
    return out


def resources(text):
    """{kernel name: {figure: value}} of one <unit>.resources.txt."""
    out, cur = {}, None
    for line in text.splitlines():
        m = re.search(r"remark:\s+(.*?)\s+\[-Rpass-analysis=kernel-resource-usage\]", line)
        if not m:
            continue
        key, _, value = m.group(1).partition(": ")
        if key == "Function Name":
            cur = out.setdefault(kernel_name(value), {})
        elif cur is not None:
            cur[key] = value
    return out


def compare(old, new, old_res=None, new_res=None):
    """The report lines and the number of differences of one unit; old's names go through RENAMES."""
    a = {renamed(k): v for k, v in kernels(old).items()}
    b = kernels(new)
    ra = {renamed(k): v for k, v in resources(old_res).items()} if old_res is not None and new_res is not None else {}
    rb = resources(new_res) if ra else {}
    lines, bad = [], 0
    for name in sorted(set(a) | set(b), key=show):
        if name not in a or name not in b:
            lines.append(f"{show(name)}: only in the {'first' if name in a else 'second'} directory")
            bad += 1
            continue
        x, y = a[name], b[name]
        if x != y:
            k = next((i for i, (p, q) in enumerate(zip(x, y)) if p != q), min(len(x), len(y)))
            lines.append(f"{show(name)}: DIFFERS at instruction {k} ({len(x)} against {len(y)} lines)")
            lines += [f"    - {p}" for p in x[k:k + 3]] + [f"    + {q}" for q in y[k:k + 3]]
            bad += 1
        elif ra.get(name) != rb.get(name):
            moved = {f: (ra.get(name, {}).get(f), rb.get(name, {}).get(f)) for f in set(ra.get(name, {})) | set(rb.get(name, {}))}
            lines.append(f"{show(name)}: identical instructions, RESOURCES DIFFER: " +
                         ", ".join(f"{f} {p} -> {q}" for f, (p, q) in sorted(moved.items()) if p != q))
            bad += 1
        else:
            lines.append(f"{show(name)}: identical")
    return lines, bad


def read(path):
    return open(path).read() if os.path.exists(path) else None


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    da, db = sys.argv[1:]
    units = sorted({f[:-2] for d in (da, db) for f in os.listdir(d) if f.endswith(".s")})
    bad = total = 0
    for u in units:
        old, new = read(os.path.join(da, u + ".s")), read(os.path.join(db, u + ".s"))
        if old is None or new is None:
            print(f"{u}: only in the {'second' if old is None else 'first'} directory")
            bad += 1
            continue
        lines, n = compare(old, new, read(os.path.join(da, u + ".resources.txt")), read(os.path.join(db, u + ".resources.txt")))
        for line in lines:
            print(f"{u}: {line}")
        bad += n
        total += sum(1 for line in lines if not line.startswith("    "))
    print(f"{total} kernels in {len(units)} units, {bad} differences")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
