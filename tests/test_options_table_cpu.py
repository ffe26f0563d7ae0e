"""tests/options_table.py is complete and says what it claims (no device needed): one entry per key of engine.option_keys(), one row of
INTEGRATION.md section 4 per key, every `covered_by` target an existing test that names its key, every row without a witness with a reason."""
import ast
import os
import re

import options_table as ot

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_one_entry_per_option_key(pkg):
    keys = pkg.engine.option_keys()
    assert len(keys) == len(set(keys))
    assert set(ot.TABLE) == set(keys), (sorted(set(keys) - set(ot.TABLE)), sorted(set(ot.TABLE) - set(keys)))
    assert set(ot.ABOVE) == set(keys)  # (the refusal test has a value above every option's range)


def test_options_that_act_on_two_families_have_a_row_in_each():
    """(Deleting the second row of such a key leaves the key in the table: this is what notices it.)"""
    two = {"gjk_beside_max": {"solids64", "solids32"}, "cvx_w": {"solids64", "hulls32"}, "pool_rerun": {"mm", "ms"}, "bvh_force_wide": {"mm", "ms"}}
    for key, families in two.items():
        assert {r.family for r in ot.TABLE[key]} == families, key
    for key, rows in ot.TABLE.items():
        assert len(rows) == len({getattr(r, "family", None) for r in rows}) and (len(rows) == 1 or key in two), key


def test_one_row_of_the_integration_table_per_key(pkg):
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    section = text[text.index("## 4. Tuning options"):]
    section = section[:section.index("\n### ")]
    documented = re.findall(r"^\| `([a-z0-9_]+)` \|", section, flags=re.M)
    assert len(documented) == len(set(documented))
    assert set(documented) == set(pkg.engine.option_keys()), (sorted(set(documented) ^ set(pkg.engine.option_keys())))


def _functions(path):
    src = open(path).read()
    tree = ast.parse(src)
    return {node.name: ast.get_source_segment(src, node) for node in tree.body if isinstance(node, ast.FunctionDef)}, tree


def test_covered_by_targets_exist_and_name_their_key():
    """The named test exists, and its source -- or the source of a function of the same module that it calls by name -- holds the key as a
    whole word (scene_pairs_sorted_axis does not count for scene_pairs_sorted)."""
    covered = [r for rows in ot.TABLE.values() for r in rows if isinstance(r, ot.Covered)]
    assert covered
    for row in covered:
        module, _, name = row.by.partition("::")
        path = os.path.join(HERE, module)
        assert os.path.isfile(path), row.by
        functions, _ = _functions(path)
        assert name.startswith("test_") and name in functions, row.by
        seen, todo = set(), [name]
        while todo:  # the test and the helpers of its module that it calls, directly or through one another
            f = todo.pop()
            seen.add(f)
            calls = {n.func.id for n in ast.walk(ast.parse(functions[f])) if isinstance(n, ast.Call) and isinstance(n.func, ast.Name)}
            todo += [c for c in sorted(calls) if c in functions and c not in seen and not c.startswith("test_")]
        source = "".join(functions[f] for f in sorted(seen))
        assert re.search(r"(?<![a-z0-9_])%s(?![a-z0-9_])" % re.escape(row.key), source), "%s does not name %s" % (row.by, row.key)
        assert "tobytes()" in source or "_same(" in source or "compare_records(" in source, "%s compares no bytes" % row.by


def test_rows_are_well_formed():
    for key, rows in ot.TABLE.items():
        assert rows, key
        if any(isinstance(r, ot.Covered) for r in rows):
            assert len(rows) == 1, key
            continue
        for r in rows:
            assert r.family in ot.FAMILIES and set(r.calls or ()) <= set(ot.FAMILIES[r.family]), key
            # bytes everywhere; "decisions" at the named values of fp64 mesh x mesh collide() alone ("judge" is used by no row)
            assert set(r.decisions_at) <= set(r.values) and (not r.decisions_at or (r.family == "mm" and "mm_collide" in (r.calls or ot.FAMILIES["mm"]))), key
            assert (r.threshold is None) != (not r.values), "%s: values or a threshold" % key
            assert r.witness is not None or (r.why and len(r.why) > 20), "%s: a row without a witness says why" % key
            if r.witness is None:  # only options that move work between streams
                assert key in ("mesh_prio", "epa64_two_streams", "epa_records_aside", "shape_finish_aside", "bvh_walk_early_coop"), key
            assert r.needs_ab == (r.refused is not None), key
        # at least two values run on the device: the default (the run compared against) and one more
        assert all(r.values or r.threshold for r in rows), key
