"""The cases of tests/test_node_body_gpu.py reach every field the node body of the fused walk
(walk_fused.h) branches on: decoded from ``Plan.records(groups)``, no device.  A field that the
word sets do not produce is a failure of the word sets - nothing here skips."""
import numpy as np

import test_node_body_gpu as tn

F_CHAIN, F_CHILDREN, F_SLOW, F_NEED1, F_NEED2, F_EMIT = 1, 2, 4, 8, 16, 32      # csrc/walk_types.h
SENTINEL = 0xff


def _decode(recs):
    """Per node of a (records, 16) table: level, flags, factor count, output rows; and the groups."""
    level = recs[:, 0] & 0xff
    node = level != SENTINEL
    return dict(level=level[node], flags=(recs[:, 0] >> 8)[node], nf=(recs[:, 1] & 0xffff)[node],
                ne=recs[:, 6][node], fac_begin=recs[:, 12][node]), int((~node).sum())


def test_cases_cover_the_record_fields():
    import fruits_amd as fr
    seen = set()
    done = set()
    for case in tn.CASES:
        key = (case["words"], case["weighting"], case["semiring"], case["single"], case["groups"])
        if key in done:
            continue
        done.add(key)
        words = tn.words_of(case)
        iss = tn.make_iss(fr, case)
        plan = iss._plan(0, len(words))
        recs, groups = _decode(plan.records(max(case["groups"], 1)))
        assert groups == max(case["groups"], 1), (case["name"], groups)
        if groups == 2:
            seen.add("two groups")
        for lv, fl, nf, ne in zip(recs["level"], recs["flags"], recs["nf"], recs["ne"]):
            seen.add("level %d" % min(lv, 2))
            seen.add("chain" if fl & F_CHAIN else "no chain")
            if fl & F_SLOW:
                seen.add("slow: more than four factors" if nf > 4 else "slow: %d factors" % nf)
            else:
                assert 1 <= nf <= 4
                seen.add("inline %d" % nf)
            seen.add("emit %d" % min(ne, 3) if fl & F_EMIT else "no emit")
            assert bool(fl & F_EMIT) == (ne > 0)
            seen.add("need2" if fl & F_NEED2 else "no need2")
            if fl & F_NEED2:
                assert case["weighting"] == "indices" and fl & F_CHILDREN
    want = {"level 0", "level 1", "level 2", "chain", "no chain", "slow: more than four factors",
            "inline 1", "inline 2", "inline 3", "inline 4", "no emit", "emit 1", "emit 2", "emit 3",
            "need2", "no need2", "two groups"}
    assert want <= seen, sorted(want - seen)
    # the reciprocal letter: a node on the factor table with no more than four factors
    assert any(s.startswith("slow: ") and s != "slow: more than four factors" for s in seen), sorted(seen)


def test_a_repeated_word_names_three_rows_of_one_node():
    """SINGLE mode, a word three times: one node with three output rows, the third from the
    emit-row table (the first two are inline in the record)."""
    import fruits_amd as fr
    case = next(c for c in tn.CASES if c["single"] and c["words"] == "single")
    recs, _ = _decode(tn.make_iss(fr, case)._plan(0, len(tn.words_of(case))).records(1))
    emitting = recs["ne"][(recs["flags"] & F_EMIT) != 0]
    assert np.count_nonzero(emitting >= 3) == 1 and np.count_nonzero(recs["ne"] == 0) > 0
