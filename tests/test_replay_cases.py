"""The capture table of tests/replay_cases.py held to pgl_amd.ops without a GPU: the three name sets partition the module's
public callables, every host read and every atomic that is quoted exists where it is quoted, and no CAPTURABLE op reads a device
value back in its own body unless the table says under which argument.  A new op cannot land without someone deciding which set it
belongs to."""
import inspect
import os

import replay_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_READS = (".item()", ".tolist()", ".nonzero(", ".cpu()", ".numpy()")
# CAPTURABLE ops whose body holds a host read behind an argument: name -> (text of the line, the call that avoids it)
READS_BEHIND_AN_ARGUMENT = {
    "segment_reduce": ("num_segments = int(segment_ids[-1].item()) + 1 if n else 0", "pass num_segments"),
}


def _ops():
    import pgl_amd.ops as ops
    return ops


def _sets():
    return RC.public_callables(_ops()), RC.CAPTURABLE, RC.NOT_CAPTURABLE, RC.NO_DEVICE_WORK


def test_the_three_sets_partition_the_public_callables():
    errors = RC.partition_errors(*_sets())
    assert not errors, "\n".join(errors)


def test_a_name_in_no_set_or_in_two_is_reported():
    public, capturable, host_read, no_work = _sets()
    missing = "%s is in none of CAPTURABLE, NOT_CAPTURABLE, NO_DEVICE_WORK: decide where it belongs"
    assert RC.partition_errors(public + ["brand_new_op"], capturable, host_read, no_work) == [missing % "brand_new_op"]
    for victim in ("aggregate", "csr_build", "set_option"):
        errors = RC.partition_errors(public, set(capturable) - {victim}, {k: v for k, v in host_read.items() if k != victim},
                                     set(no_work) - {victim})
        assert errors == [missing % victim]
    assert RC.partition_errors(public, capturable, host_read, set(no_work) | {"aggregate"}) == \
        ["aggregate is listed twice: CAPTURABLE and NO_DEVICE_WORK"]
    assert RC.partition_errors(public, capturable, host_read, set(no_work) | {"no_such_op"}) == \
        ["no_such_op is listed but is no public callable of pgl_amd.ops"]


def _source_of(where):
    if where.startswith("csrc/"):
        with open(os.path.join(ROOT, "pgl_amd", where)) as f:
            return f.read()
    return inspect.getsource(getattr(_ops(), where))


def test_every_host_read_is_where_its_reason_says():
    ops = _ops()
    for name, entry in RC.NOT_CAPTURABLE.items():
        assert len(entry) == 3 and all(isinstance(s, str) and s.strip() for s in entry), "%s: (where, line, why) expected" % name
        where, line, why = entry
        assert line in _source_of(where), "%s: %r is not in %s any more -- find the host read again" % (name, line, where)
        if not where.startswith("csrc/") and where != name:        # the read is in a helper: the op must reach it
            reach = {"slice_table": ("slice_plan(", "slice_plan"), "slice_plan": ("_build_slice_plan(", "slice_plan")}.get(name)
            if reach is None:
                assert where + "(" in inspect.getsource(getattr(ops, name)), (name, where)
            else:
                assert reach[0] in inspect.getsource(getattr(ops, name)), (name, where)
    assert "_build_slice_plan(" in inspect.getsource(ops.slice_plan)


def test_no_capturable_op_reads_a_device_value_back_in_its_own_body():
    ops = _ops()
    for name in sorted(RC.CAPTURABLE):
        src = inspect.getsource(getattr(ops, name))
        allowed = READS_BEHIND_AN_ARGUMENT.get(name)
        if allowed is not None:
            assert allowed[0] in src, "%s: the read %r has left the source: drop the exception" % (name, allowed[0])
            src = src.replace(allowed[0], "")
        code = "\n".join(l.split("#")[0] for l in src.split('"""')[-1].splitlines())       # (the body after the docstring, comments cut)
        found = [r for r in HOST_READS if r in code]
        assert not found, "%s is listed CAPTURABLE but its body reads back with %s" % (name, found)
    assert set(READS_BEHIND_AN_ARGUMENT) <= set(RC.CAPTURABLE)


def test_every_quoted_float_atomic_exists_and_belongs_to_a_capturable_op():
    for name, (where, line) in RC.FLOAT_ATOMICS.items():
        assert name in RC.CAPTURABLE, name
        assert line in _source_of(where), "%s: the atomic %r is not in %s any more" % (name, line, where)
    # the only float atomic add in the library's sources is a quoted one
    csrc = os.path.join(ROOT, "pgl_amd", "csrc")
    quoted = {line for _, line in RC.FLOAT_ATOMICS.values()}
    for fn in sorted(os.listdir(csrc)):
        if fn.endswith((".hip", ".hpp", ".cpp")):
            with open(os.path.join(csrc, fn)) as f:
                for l in f:
                    if "unsafeAtomicAdd(" in l and not l.lstrip().startswith("//"):
                        assert any(q in l for q in quoted), "%s: a float atomic that FLOAT_ATOMICS does not quote: %s" % (fn, l.strip())


def test_every_capturable_op_has_a_side_stream_case_or_is_named_as_having_none():
    public = set(RC.public_callables(_ops()))
    covered = set()
    for case in RC.side_stream_cases():
        assert case.ops and set(case.ops) <= public, "%s names %s" % (case.name, sorted(set(case.ops) - public))
        assert set(case.ops) <= set(RC.CAPTURABLE), "%s drives %s, which the table does not call CAPTURABLE" % (case.name, case.ops)
        assert case.bounded == any(o in RC.FLOAT_ATOMICS for o in case.ops), "%s: bounded exactly when it runs a float atomic" % case.name
        assert not case.bounded or case.check is not None
        covered |= set(case.ops)
    assert not covered & set(RC.NO_SIDE_STREAM_CASE), sorted(covered & set(RC.NO_SIDE_STREAM_CASE))
    assert covered | set(RC.NO_SIDE_STREAM_CASE) == set(RC.CAPTURABLE), sorted(set(RC.CAPTURABLE) - covered - set(RC.NO_SIDE_STREAM_CASE))


def test_ops_that_need_a_warm_index_reach_the_helper_that_reads():
    ops = _ops()
    for name, (helper, why) in RC.NEEDS_WARM_INDEX.items():
        assert name in RC.CAPTURABLE and why.strip()
        assert helper + "(" in inspect.getsource(getattr(ops, name)), (name, helper)
        assert helper in RC.NOT_CAPTURABLE
