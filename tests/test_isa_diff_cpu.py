"""tools/isa_diff.py on plain strings: what it ignores, what it reports and under which kernel."""
import importlib.util
import os

_spec = importlib.util.spec_from_file_location(
    "isa_diff", os.path.join(os.path.dirname(__file__), "..", "tools", "isa_diff.py"))
isa_diff = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(isa_diff)


def _kernel(name, body, vgprs=12):
    return f"""\t.text
\t.protected\t{name}
\t.globl\t{name}
\t.type\t{name},@function
{name}:                                   ; @{name}
; %bb.0:
{body}
\ts_endpgm
.Lfunc_end_{name}:
\t.section\t.rodata,"a",@progbits
\t.amdhsa_kernel {name}
\t\t.amdhsa_next_free_vgpr {vgprs}
\t.end_amdhsa_kernel
\t.text
\t.size\t{name}, .Lfunc_end_{name}-{name}
"""


def _meta(names, vgprs=12):
    items = "".join(f"""  - .agpr_count:     0
    .args:
      - .address_space:  global
        .offset:         0
    .name:           {n}
    .private_segment_fixed_size: 0
    .sgpr_count:     20
    .vgpr_count:     {vgprs}
    .vgpr_spill_count: 0
""" for n in names)
    return f"\t.amdgpu_metadata\n---\namdhsa.kernels:\n{items}...\n\t.end_amdgpu_metadata\n"


def _listing(bodies, cuid="aaaa", ident="clang 1", note="first"):
    text = "\t.file\t\"x.hip\"\n" + "".join(_kernel(n, b) for n, b in bodies.items())
    text += f"\t.type\t__hip_cuid_{cuid},@object\n__hip_cuid_{cuid}:\n\t.byte 0\n\t.size\t__hip_cuid_{cuid}, 1\n"
    text += f"\t.ident\t\"{ident}\"\n ; {note}\n"
    return text + _meta(bodies)


A = "\tv_add_f32_e32 v0, v1, v2 ; a comment\n\t.loc\t1 10 3\n\tv_mul_f32_e32 v3, v0, v0"
B = "\tv_mov_b32_e32 v0, 0"


def _run(a, b):
    out = []
    return isa_diff.diff_listings("tu", a, b, out.append), out


def test_comments_ident_and_cuid_do_not_count():
    a = _listing({"k1": A, "k2": B})
    b = _listing({"k1": A.replace("a comment", "another").replace("1 10 3", "1 99 1"), "k2": B},
                 cuid="bbbb", ident="clang 2", note="second")
    assert a != b
    bad, out = _run(a, b)
    assert bad == 0
    assert sorted(out) == ["tu: (file scope): identical", "tu: k1: identical", "tu: k2: identical"]


def test_one_changed_instruction_is_reported_under_its_kernel_only():
    a = _listing({"k1": A, "k2": B})
    b = _listing({"k1": A.replace("v_mul_f32_e32 v3", "v_mul_f32_e32 v4"), "k2": B})
    bad, out = _run(a, b)
    assert bad == 1
    heads = [l.split(" DIFFERENT")[0] + " DIFFERENT" if " DIFFERENT" in l else l for l in out if l.startswith("tu: ")]
    assert sorted(heads) == ["tu: (file scope): identical", "tu: k1: DIFFERENT", "tu: k2: identical"]
    text = "\n".join(out)
    assert "v_mul_f32_e32 v3, v0, v0" in text and "v_mul_f32_e32 v4, v0, v0" in text
    assert text.count(".vgpr_count:12") == 2 and ".private_segment_fixed_size:0" in text and ".vgpr_spill_count:0" in text


def test_kernel_on_one_side_only_is_reported():
    a = _listing({"k1": A, "k2": B})
    b = _listing({"k1": A})
    for x, y, side in ((a, b, "first"), (b, a, "second")):
        bad, out = _run(x, y)
        assert bad == 1
        assert f"tu: k2: only in {side}" in out and "tu: k1: identical" in out


def test_main_pairs_listings_by_name_and_sets_the_exit_status(tmp_path, capsys):
    da, db = tmp_path / "a", tmp_path / "b"
    da.mkdir(), db.mkdir()
    (da / ("x" + isa_diff.SUFFIX)).write_text(_listing({"k1": A}))
    (db / ("x" + isa_diff.SUFFIX)).write_text(_listing({"k1": A}, cuid="cccc"))
    assert isa_diff.main(["isa_diff", str(da), str(db)]) == 0
    (db / ("y" + isa_diff.SUFFIX)).write_text(_listing({"k2": B}))
    assert isa_diff.main(["isa_diff", str(da), str(db)]) == 1
    assert "y: listing only in second" in capsys.readouterr().out
