"""The shared output-writer stimulus (tests/output_writer_stimulus.py), run through the restatement alone: it has to reach
every branch the restatement counts, and put at least three different output lengths into one push.  A branch it leaves
unvisited is a failure here, so that the GPU comparison cannot pass on ground it never walked."""
import numpy as np
import pytest

import output_writer_oracle as O
import output_writer_stimulus as stim


@pytest.fixture(scope="module")
def runs():
    out = {}
    for name in stim.CONFIGS:
        lim = stim.limits(name)
        out[name] = O.run_sequence(stim.sequence(name), stim.N_STREAMS, rate=float(lim["rate"]), capacity=lim["capacity"],
                                   center=lim["center"], hard=lim["hard"], fade=lim["fade"])
    return out


def test_every_branch_is_visited(runs):
    total = {k: 0 for k in O.BRANCHES}
    for name, steps in runs.items():
        # a reset clears the branch counters too: add what each stretch between resets reached
        last = None
        for step, push in zip(steps, stim.sequence(name)):
            if ("reset",) in push["pre"] and last is not None:
                for k in O.BRANCHES:
                    total[k] += last[k]
            last = step["branches"]
        for k in O.BRANCHES:
            total[k] += last[k]
    unvisited = [k for k, v in total.items() if v == 0]
    assert not unvisited, unvisited


@pytest.mark.parametrize("name", ["derived_48k", "limits_128_256_4"])
def test_one_push_holds_at_least_three_output_lengths(runs, name):
    best = max(len(set(step["meters"]["out_len"].tolist())) for step in runs[name])
    assert best >= 3, best


def test_roles_share_a_launch(runs):
    """expand, pass-through, compress, emergency, short write and zero free space among the streams of one push"""
    push = stim.sequence("derived_48k")[0]
    m = runs["derived_48k"][0]["meters"]
    n = push["x"].shape[1]
    lim = stim.limits("derived_48k")
    written = np.asarray([r.size for r in runs["derived_48k"][0]["rows"]])
    assert (m["out_len"] > n).any() and (m["out_len"] == n).any() and (m["out_len"] < n).any()
    assert (m["ratio"] == np.float32(1.06)).any()
    assert ((written < m["out_len"]) & (written > 0)).any() and ((written == 0) & (push["fill"] == lim["capacity"])).any()


def test_fade_straddles_two_and_three_pushes(runs):
    """a re-armed fade that is still running after the next push, and after the one behind it"""
    for name in ("derived_48k",):
        fade = np.stack([step["meters"]["fade_remaining"] for step in runs[name]])
        full = stim.limits(name)["fade"]
        running = (fade > 0) & (fade < full)
        assert (running[1:] & running[:-1]).any(), "no fade runs across two pushes"
        assert (running[2:] & running[1:-1] & running[:-2]).any(), "no fade runs across three pushes"
