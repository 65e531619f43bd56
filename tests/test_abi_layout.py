"""The drop-in boundary, checked against the reference's own headers.

The components are compiled against a layout mirror of the plugin ABI
(zhpe-ompi_amd/mca/mx_ompi_abi.h).  Here every mirrored struct is compared
member by member with the reference:

* opal_object_t, mca_base_component_2_1_0_t / _data_t
  (opal/mca/mca.h:285-342), ompi_op_base_component_1_0_0_t and
  ompi_op_base_module_1_0_0_t (ompi/mca/op/op.h:331-378): offsetof / sizeof
  as a probe program that includes the reference's real headers reports them;
* mca_coll_base_module_2_3_0_t (ompi/mca/coll/coll.h:504-604) and
  mca_coll_base_component_2_0_0_t (:471-481): coll.h needs the generated
  mpi.h, so its member list is read from the header text -- every member
  after `opal_object_t super` is one pointer, so a member's offset is
  sizeof(opal_object_t) + 8 x its position.

The reference's side of every comparison (member names, offsets, sizes, the
names its headers declare) is recorded in tests/golden/ref_abi_layout.json
by oracle/record_reference_facts.py, which reads a reference tree with
tests/ref_abi.py; the mirror's side is compiled and probed here, so these
tests need no reference tree.  Compiling the components themselves against
the reference's headers (-DMX_OMPI_REAL) needs such a tree and is described
in INTEGRATION.md section 1.
"""
import os
import re

from ref_abi import compile_run, load, probe_src

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ABI = os.path.join(ROOT, "zhpe-ompi_amd", "mca")
REFERENCE = load()


def test_op_framework_and_mca_base_layouts_match_reference(tmp_path):
    items = [tuple(i) for i in REFERENCE["op_mca"]["items"]]
    real = REFERENCE["op_mca"]["real"]
    assert set(real) == {i[0] for i in items}
    mirror = compile_run(tmp_path, "mirror", probe_src(["mx_ompi_abi.h"], items), [ABI, os.path.join(ROOT, "include")])
    assert real["sizeof opal_object_t"] == 16, real     # OPAL_ENABLE_DEBUG = 0 layout
    diff = {k: (real[k], mirror[k]) for k in real if real[k] != mirror[k]}
    assert not diff, f"mirror differs from the reference headers (reference, mirror): {diff}"


def test_coll_module_and_component_layouts_match_reference(tmp_path):
    mods = REFERENCE["coll"]["module_members"]
    comps = REFERENCE["coll"]["component_members"]
    assert mods[0] == "super" and mods[1] == "coll_module_enable" and mods[-1] == "base_data"
    assert len(mods) == 1 + 1 + 3 * 17 + 3 * 5 + 3 + 1, len(mods)      # coll.h:504-604
    assert comps == ["collm_version", "collm_data", "collm_init_query", "collm_comm_query"]
    items = [(f"m.{x}", "mca_coll_base_module_t", x) for x in mods] + \
            [(f"c.{x}", "mca_coll_base_component_2_0_0_t", x) for x in comps] + \
            [("sizeof m", "mca_coll_base_module_t", None)]
    mirror = compile_run(tmp_path, "mirror_coll", probe_src(["mx_ompi_abi.h"], items),
                         [ABI, os.path.join(ROOT, "include")])
    real = REFERENCE["coll"]["real"]     # sizeof opal_object_t / mca_base_component_t / _data_t
    for i, x in enumerate(mods):
        exp = 0 if i == 0 else real["obj"] + 8 * (i - 1)
        assert mirror[f"m.{x}"] == exp, (x, mirror[f"m.{x}"], exp)
    assert mirror["sizeof m"] == real["obj"] + 8 * (len(mods) - 1)
    data_off = real["comp"]
    fn_off = (data_off + real["data"] + 7) // 8 * 8
    assert [mirror[f"c.{x}"] for x in comps] == [0, data_off, fn_off, fn_off + 8]


# ---------------------------------------------------------------------------
# mca/mx_ompi_host_real.c: the real-tree host table (round 4)
# ---------------------------------------------------------------------------
HOST_REAL = os.path.join(ABI, "mx_ompi_host_real.c")


def test_real_host_table_uses_only_internals_the_reference_declares():
    """Every Open MPI internal the table calls is declared in the reference's
    headers (a function prototype, a macro, or -- ompi_op_ddt_map -- an
    extern array), and every struct member it reads exists in the struct the
    reference defines: the table would compile inside a configured tree
     up to the signatures the headers give."""
    src = open(HOST_REAL).read()
    body = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = REFERENCE["declared"]
    calls = set(re.findall(r"\b((?:ompi|opal|mca_base)_[A-Za-z0-9_]+)\s*\(", body))
    macros = set(re.findall(r"\b((?:OBJ|OMPI_REQUEST|OMPI_COMM)_[A-Z_]+)\b", body))
    assert {"ompi_comm_rank", "ompi_datatype_type_size", "opal_convertor_pack", "mca_base_var_find"} <= calls
    missing = sorted(calls - set(declared["functions"]))
    assert not missing, f"called but not declared by the reference: {missing}"
    missing = sorted(macros - set(declared["macros"]))
    assert not missing, f"macros / enumerators not defined by the reference: {missing}"
    assert declared["ompi_op_ddt_map_is_an_extern_int_array"] is True          # op.h:246
    members = {
        "ompi/op/op.h": ["o_f_to_c_index", "o_flags", "o_func", "o_3buff_intrinsic"],
        "ompi/datatype/ompi_datatype.h": ["super", "id"],
        "opal/datatype/opal_datatype.h": ["opt_desc", "desc", "size", "lb", "ub", "used"],
        "ompi/communicator/communicator.h": ["c_coll"],
        "ompi/request/request.h": ["req_status", "req_start", "req_free", "req_type", "req_state"],
        "opal/mca/base/mca_base_var.h": ["mbv_type"],
    }
    for hdr, mems in members.items():
        for m in mems:
            assert m in declared["members"][hdr], f"{hdr} has no member {m}"
        for m in mems:
            assert re.search(r"(->|\.)" + m + r"\b", body), f"{m} listed but unused"


# ---------------------------------------------------------------------------
# round 5: the convertor hook and the BTL GPU RDMA slots (VERDICT r4 missing 3, 4)
# ---------------------------------------------------------------------------
def test_convertor_and_datatype_layouts_match_reference(tmp_path):
    """opal_convertor_t / opal_datatype_t / dt_type_desc_t / dt_stack_t of
    the mirror (mca/mx_opal_convertor_abi.h) vs the reference's own headers
    (an x86-64 gcc build without CUDA: cbmemcpy / stream are not there)."""
    items = [tuple(i) for i in REFERENCE["convertor"]["items"]]
    real = REFERENCE["convertor"]["real"]
    assert set(real) == {i[0] for i in items}
    for typ in ("opal_convertor_t", "dt_stack_t", "opal_datatype_t", "dt_type_desc_t"):
        assert f"sizeof {typ}" in real and sum(k.startswith(typ + ".") for k in real) >= 2, typ
    mirror = compile_run(tmp_path, "mirror_conv", probe_src(["mx_opal_convertor_abi.h"], items),
                         [ABI, os.path.join(ROOT, "include")])
    diff = {k: (real[k], mirror[k]) for k in real if real[k] != mirror[k]}
    assert not diff, f"mirror differs from the reference headers (reference, mirror): {diff}"


def test_btl_module_layout_matches_reference(tmp_path):
    """mca_btl_base_module_t offsets as btl.h's text gives them (every member
    is a size_t, a uint32_t, a pointer or the 256-byte padding; the CUDA
    members are left out, as an MI355X build has neither: ref_abi._btl_offsets)."""
    ref = REFERENCE["btl"]["offsets"]
    assert "btl_get" in ref and "btl_flush" in ref and "padding" in ref
    assert "btl_cuda_eager_limit" not in ref
    items = [(k, "mca_btl_base_module_t", k) for k in ref if k != "sizeof"] + \
            [("sizeof", "mca_btl_base_module_t", None)]
    mirror = compile_run(tmp_path, "mirror_btl", probe_src(["mx_btl_abi.h"], items),
                         [ABI, os.path.join(ROOT, "include")])
    diff = {k: (ref[k], mirror[k]) for k in ref if ref[k] != mirror[k]}
    assert not diff, f"BTL module mirror differs from btl.h (reference, mirror): {diff}"
    # the slot signatures: the get / put / register typedefs restated from the header text
    for typedef in ("mca_btl_base_module_get_fn_t", "mca_btl_base_module_put_fn_t",
                    "mca_btl_base_module_register_mem_fn_t", "mca_btl_base_module_deregister_mem_fn_t",
                    "mca_btl_base_module_flush_fn_t", "mca_btl_base_rdma_completion_fn_t"):
        assert typedef in REFERENCE["btl"]["fn_typedefs"]
    assert REFERENCE["btl"]["get_fn_params"] == [
        "btl", "endpoint", "local_address", "remote_address", "local_handle", "remote_handle", "size", "flags",
        "order", "cbfunc", "cbcontext", "cbdata"]
