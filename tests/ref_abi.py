"""What tests/test_abi_layout.py needs to know about the reference's headers
(TEST INFRASTRUCTURE).

record(ref_dir) reads it from a reference tree: struct member lists from the
header text, offsetof / sizeof reported by probe programs that include the
real headers (tests/abi/opal_config.h stands for the configure output of an
x86-64 gcc build), the names the headers declare.  Only names and numbers
are kept -- nothing of the reference's text.  oracle/record_reference_facts.py
stores the result as tests/golden/ref_abi_layout.json; load() returns it, so
the tests need no reference tree.
"""
import json
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ref_abi_layout.json")

# headers whose struct members mca/mx_ompi_host_real.c reads
MEMBER_HEADERS = ["ompi/op/op.h", "ompi/datatype/ompi_datatype.h", "opal/datatype/opal_datatype.h",
                  "ompi/communicator/communicator.h", "ompi/request/request.h", "opal/mca/base/mca_base_var.h"]


def load():
    with open(GOLDEN) as f:
        return json.load(f)


def struct_members(path, tag):
    """Member names of `struct tag { ... };` in a C header, in order."""
    text = open(path).read()
    m = re.search(r"struct\s+" + re.escape(tag) + r"\s*\{", text)
    assert m, (path, tag)
    depth, i = 1, m.end()
    while depth:
        depth += {"{": 1, "}": -1}.get(text[i], 0)
        i += 1
    body = text[m.end():i - 1]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    body = re.sub(r"//[^\n]*", "", body)
    body = "\n".join(ln for ln in body.splitlines() if not ln.strip().startswith("#"))
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        decl = re.sub(r"\[[^\]]*\]", "", decl)
        names.append(re.findall(r"[A-Za-z_]\w*", decl)[-1])
    return names


def compile_run(tmp_path, name, src, incs, defs=()):
    c = os.path.join(str(tmp_path), f"{name}.c")
    exe = os.path.join(str(tmp_path), name)
    with open(c, "w") as f:
        f.write(src)
    cmd = ["gcc", "-std=gnu11", "-w", *[f"-D{d}" for d in defs], *[f"-I{i}" for i in incs], c, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    return json.loads(out)


def probe_src(includes, items):
    """items: (key, struct type, member or None)"""
    lines = ["#include <stddef.h>", "#include <stdio.h>", *[f'#include "{h}"' for h in includes],
             "int main(void) {", '  printf("{");']
    for k, (key, typ, mem) in enumerate(items):
        expr = f"sizeof({typ})" if mem is None else f"offsetof({typ}, {mem})"
        sep = "" if k == 0 else ","
        lines.append(f'  printf("{sep}\\"{key}\\": %zu", (size_t)({expr}));')
    lines += ['  printf("}\\n");', "  return 0;", "}"]
    return "\n".join(lines)


def _op_mca_items(ref):
    items = [("sizeof opal_object_t", "opal_object_t", None),
             ("sizeof mca_base_component_t", "mca_base_component_t", None),
             ("sizeof mca_base_component_data_t", "mca_base_component_data_t", None)]
    for typ, tag in (("mca_base_component_t", "mca_base_component_2_1_0_t"),):
        for mem in struct_members(os.path.join(ref, "opal", "mca", "mca.h"), tag):
            items.append((f"{typ}.{mem}", typ, mem))
    for typ, tag in (("ompi_op_base_component_1_0_0_t", "ompi_op_base_component_1_0_0_t"),
                     ("ompi_op_base_module_1_0_0_t", "ompi_op_base_module_1_0_0_t")):
        for mem in struct_members(os.path.join(ref, "ompi", "mca", "op", "op.h"), tag):
            items.append((f"{typ}.{mem}", typ, mem))
        items.append((f"sizeof {typ}", typ, None))
    return items


def _convertor_items(ref):
    conv_h = os.path.join(ref, "opal", "datatype", "opal_convertor.h")
    dt_h = os.path.join(ref, "opal", "datatype", "opal_datatype.h")
    items = []
    for typ, hdr in (("opal_convertor_t", conv_h), ("dt_stack_t", conv_h), ("opal_datatype_t", dt_h),
                     ("dt_type_desc_t", dt_h)):
        mems = struct_members(hdr, typ)
        if typ == "opal_convertor_t":        # OPAL_CUDA_SUPPORT = 0: cbmemcpy / stream are not there
            mems = [m for m in mems if m not in ("cbmemcpy", "stream")]
        for mem in mems:
            items.append((f"{typ}.{mem}", typ, mem))
        items.append((f"sizeof {typ}", typ, None))
    return items


def _btl_offsets(text):
    """mca_btl_base_module_t offsets from btl.h's text (the header needs
    configure-generated threads headers): every member is a size_t, a
    uint32_t, a pointer (function or object) or the 256-byte padding; the
    CUDA members (#if OPAL_CUDA_GDR_SUPPORT / OPAL_CUDA_SUPPORT) are left out,
    as an MI355X build has neither."""
    m = re.search(r"struct\s+mca_btl_base_module_t\s*\{", text)
    depth, i = 1, m.end()
    while depth:
        depth += {"{": 1, "}": -1}.get(text[i], 0)
        i += 1
    body = re.sub(r"/\*.*?\*/", "", text[m.end():i - 1], flags=re.S)
    # drop the conditional CUDA blocks
    body = re.sub(r"#if OPAL_CUDA[^\n]*\n.*?#endif[^\n]*\n", "", body, flags=re.S)
    off, out = 0, {}
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        name = re.findall(r"[A-Za-z_]\w*", re.sub(r"\[[^\]]*\]", "", decl))[-1]
        if "[" in decl:                                  # unsigned char padding[256]
            size, align = int(re.search(r"\[(\d+)\]", decl).group(1)), 1
        elif decl.startswith("uint32_t"):
            size = align = 4
        else:                                            # size_t, pointers, *_fn_t
            size = align = 8
        off = (off + align - 1) // align * align
        out[name] = off
        off += size
    out["sizeof"] = (off + 7) // 8 * 8
    return out


def _declared_names(ref):
    """Names the reference's headers declare, as far as mx_ompi_host_real.c can
    use them: function-like names (prototype or macro) with an ompi_ / opal_ /
    mca_base_ prefix, the OBJ_ / OMPI_REQUEST_ / OMPI_COMM_ macros and
    enumerators, and the member-like names of MEMBER_HEADERS."""
    hdrs = {}
    for sub in ("ompi", "opal"):
        for dp, _, fns in os.walk(os.path.join(ref, sub)):
            for fn in fns:
                if fn.endswith(".h"):
                    p = os.path.join(dp, fn)
                    hdrs[os.path.relpath(p, ref)] = open(p, errors="replace").read()
    alltext = "\n".join(hdrs.values())
    functions = sorted(set(re.findall(r"\b((?:ompi|opal|mca_base)_[A-Za-z0-9_]+)\s*\(", alltext)))
    cands = sorted(set(re.findall(r"\b((?:OBJ|OMPI_REQUEST|OMPI_COMM)_[A-Z_]+)\b", alltext)))
    macros = [m for m in cands if re.search(r"(#\s*define\s+" + m + r"\b|\b" + m + r"\b\s*[,=}])", alltext)]
    members = {}
    for hdr in MEMBER_HEADERS:
        text = hdrs[hdr]
        names = set(re.findall(r"[\s\*]([A-Za-z_]\w*)\s*(?:;|\[|:)", text))
        names |= set(re.findall(r"\(\s*\*\s*([A-Za-z_]\w*)\s*\)", text))
        members[hdr] = sorted(names)
    return {"functions": functions, "macros": macros, "members": members,
            "ompi_op_ddt_map_is_an_extern_int_array": bool(
                re.search(r"OMPI_DECLSPEC\s+extern\s+int\s+ompi_op_ddt_map\s*\[", hdrs["ompi/op/op.h"]))}


def record(ref, tmp_path):
    """Everything load() returns, read from the reference tree at `ref`."""
    incs = [os.path.join(ROOT, "tests", "abi"), ref, os.path.join(ref, "opal", "include"),
            os.path.join(ref, "ompi", "include")]
    coll_h = os.path.join(ref, "ompi", "mca", "coll", "coll.h")
    btl_text = open(os.path.join(ref, "opal", "mca", "btl", "btl.h")).read()
    op_items, conv_items = _op_mca_items(ref), _convertor_items(ref)
    get_fn = re.search(r"typedef int \(\*mca_btl_base_module_get_fn_t\)\s*\((.*?)\);", btl_text, re.S).group(1)
    return {
        "op_mca": {"items": op_items,
                   "real": compile_run(tmp_path, "real", probe_src(["opal/mca/mca.h", "ompi/mca/op/op.h"], op_items),
                                       incs)},
        "coll": {"module_members": struct_members(coll_h, "mca_coll_base_module_2_3_0_t"),
                 "component_members": struct_members(coll_h, "mca_coll_base_component_2_0_0_t"),
                 "real": compile_run(tmp_path, "real_base",
                                     probe_src(["opal/class/opal_object.h", "opal/mca/mca.h"], [
                                         ("obj", "opal_object_t", None), ("comp", "mca_base_component_t", None),
                                         ("data", "mca_base_component_data_t", None)]), incs)},
        "convertor": {"items": conv_items,
                      "real": compile_run(tmp_path, "real_conv",
                                          probe_src(["opal/datatype/opal_convertor.h"], conv_items), incs)},
        "btl": {"offsets": _btl_offsets(btl_text),
                "fn_typedefs": sorted(set(re.findall(r"\bmca_btl_base_\w+_fn_t\b", btl_text))),
                "get_fn_params": [p.strip().split()[-1].lstrip("*") for p in get_fn.replace("\n", " ").split(",")]},
        "declared": _declared_names(ref),
    }
