"""Per-row sampling, host side: the float64 restatement of the rule against hand cases, the tolerant checker's
ability to fail (a nucleus one level short or long, a token one member early or late), a host model of the device
arithmetic passing it, and serve's RunConfig validation and request seeds."""
import numpy as np
import pytest

import row_sampling_ref as ref
from distributed_inference_demo_amd.serve import RunConfig, request_seed


def _u_for(target_u, seed_range=4096):
    """A (seed, pos) whose u is close to target_u (searching seeds at position 3)."""
    best = min(range(seed_range), key=lambda s: abs(ref.draw_u24(s, 3) / 2.0 ** 24 - target_u))
    return best, 3


def test_reference_hand_cases():
    # weights at temperature 1 relative to the max: 1, 1/2, 1/4, 1/4, 1/8 (index order shuffled)
    l = np.log(np.array([0.25, 1.0, 0.125, 0.5, 0.25])).astype(np.float32)
    r = ref.reference(l, 0, 1.0, 1.0, 5, 0)
    assert (r["n_nucleus"], r["n_candidates"]) == (5, 5) and abs(r["mass_nucleus"] - 2.125) < 1e-6
    # top_p = 0.8 of 2.125 = 1.7: levels 1, 1.5, then the whole tied level of 1/4 -> 2.0
    r = ref.reference(l, 0, 0.8, 1.0, 5, 0)
    assert r["n_nucleus"] == 4 and r["t"] == pytest.approx(float(l[0])) and abs(r["mass_nucleus"] - 2.0) < 1e-6
    # top_p = 0.7 -> 1.4875: levels 1 and 1/2 suffice
    assert ref.reference(l, 0, 0.7, 1.0, 5, 0)["n_nucleus"] == 2
    # a tiny top_p keeps the top level; top_k = 1 likewise; top_k = 3 keeps the tie at the 3rd value
    assert ref.reference(l, 0, 1e-6, 1.0, 5, 0)["n_nucleus"] == 1
    assert ref.reference(l, 1, 1.0, 1.0, 5, 0)["token"] == 1
    r = ref.reference(l, 3, 1.0, 1.0, 5, 0)
    assert (r["n_candidates"], r["n_nucleus"]) == (4, 4)
    assert ref.reference(l, 9, 1.0, 1.0, 5, 0)["n_candidates"] == 5
    # temperature 0.5 squares the weights: 1, 1/4, 1/16, 1/16, 1/64
    assert abs(ref.reference(l, 0, 1.0, 0.5, 5, 0)["mass_nucleus"] - (1 + 0.25 + 0.125 + 1 / 64)) < 1e-6
    # the pick walks index order, not rank order: members of N = {0, 1, 3, 4} carry 0.25, 1, 0.5, 0.25
    for target_u, want in ((0.05, 0), (0.3, 1), (0.7, 3), (0.95, 4)):
        seed, pos = _u_for(target_u)
        assert ref.reference(l, 0, 0.8, 1.0, seed, pos)["token"] == want
    # the draw: 24 bits, keyed by (seed, position), not the generator stream of topk_sample_kernel
    assert 0 <= ref.draw_u24(7, 0) < 2 ** 24 and ref.draw_u24(7, 0) != ref.draw_u24(7, 1) != ref.draw_u24(8, 1)
    assert ref.draw_u24(7, 2 ** 20) == ref.draw_u24(7, 2 ** 20)
    # all-equal logits: the pick is floor(u24 * V / 2^24)
    eq = ref.fixture("equal", 2064)
    for pos in (0, 1, 2 ** 20):
        assert ref.reference(eq, 0, 0.9, 1.0, 11, pos)["token"] == ref.draw_u24(11, pos) * 2064 // 2 ** 24
    # -0.0 and +0.0 are one level
    z = np.array([-1.0, -0.0, 0.0, -2.0], np.float32)
    assert ref.reference(z, 1, 1.0, 1.0, 0, 0)["n_nucleus"] == 2


STATES = [(0, 0.9, 1.0), (0, 1.0, 0.7), (50, 0.95, 1.3), (5, 0.5, 1.0), (0, 1e-6, 1.0), (2100, 1.0, 2.0), (1, 1.0, 1.0),
          (0, 0.9, 0.01)]


@pytest.mark.parametrize("kind", ["normal", "tied", "spike", "equal"])
def test_checker_accepts_reference_and_device_model(kind):
    """The exact rule passes its own checker, and so does the device's arithmetic (fp32 argument, expf moved by one
    ulp either way, 2^40 fixed point) -- on every state and position, no case excluded."""
    for V in (512, 2064):
        l = ref.fixture(kind, V, seed=V)
        for i, (k, p, temp) in enumerate(STATES):
            for pos in (0, 1, 2 ** 20):
                r = ref.reference(l, k, p, temp, 90 + i, pos)
                ref.check_draw(l, k, p, temp, 90 + i, pos, r["t"], r["n_nucleus"], r["n_candidates"], r["u24"],
                               r["token"], f"reference {kind} V={V} state {i}")
                for ulp in (-1, 0, 1):
                    d = ref.device_model(l, k, p, temp, 90 + i, pos, ulp=ulp)
                    ref.check_draw(l, k, p, temp, 90 + i, pos, *d, what=f"model {kind} V={V} state {i} ulp {ulp}")


@pytest.mark.parametrize("kind", ["normal", "tied"])
def test_checker_rejects_wrong_nucleus_and_wrong_token(kind):
    """The checker must be able to fail: a nucleus one level short or one level long, and a token one nucleus member
    early or late."""
    V = 2064
    l = ref.fixture(kind, V, seed=3)
    k, p, temp, seed, pos = 0, 0.9, 1.0, 17, 5
    r = ref.reference(l, k, p, temp, seed, pos)
    levels = np.unique(l)[::-1]  # descending
    at = int(np.flatnonzero(levels == np.float32(r["t"]))[0])
    assert 0 < at < levels.size - 1

    def run(t, token):
        n = int((l >= t).sum())
        ref.check_draw(l, k, p, temp, seed, pos, t, n, r["n_candidates"], r["u24"], token)

    run(r["t"], r["token"])
    members = np.flatnonzero(l >= np.float32(r["t"]))
    j = int(np.flatnonzero(members == r["token"])[0])
    assert 0 < j < members.size - 1, "the fixture's draw must have a member on either side"
    with pytest.raises(AssertionError, match="nucleus short"):
        short = np.flatnonzero(l >= levels[at - 1])
        run(float(levels[at - 1]), int(short[0]))
    with pytest.raises(AssertionError, match="nucleus long"):
        run(float(levels[at + 1]), r["token"])
    with pytest.raises(AssertionError, match="early"):
        run(r["t"], int(members[j - 1]))
    with pytest.raises(AssertionError, match="late"):
        run(r["t"], int(members[j + 1]))
    with pytest.raises(AssertionError, match=r"\|N\|"):
        ref.check_draw(l, k, p, temp, seed, pos, r["t"], r["n_nucleus"] + 1, r["n_candidates"], r["u24"], r["token"])
    with pytest.raises(AssertionError, match="u24"):
        ref.check_draw(l, k, p, temp, seed, pos, r["t"], r["n_nucleus"], r["n_candidates"], r["u24"] ^ 1, r["token"])
    with pytest.raises(AssertionError, match="top-k level"):
        lo = float(levels[-1])
        ref.check_draw(l, 2, 1.0, temp, seed, pos, lo, V, V, r["u24"], r["token"])


def test_run_config_validation():
    c = RunConfig(sample=True, top_k=40, top_p=0.9, temperature=0.8, sample_seed=3)
    assert c.head_split is False and c.sample and (c.top_k, c.top_p, c.temperature, c.sample_seed) == (40, 0.9, 0.8, 3)
    d = RunConfig()
    assert (d.sample, d.top_k, d.top_p, d.temperature, d.sample_seed) == (False, 0, 1.0, 1.0, 0) and d.head_split
    for bad in (dict(speculate=2), dict(score=True), dict(max_length=0), dict(top_k=-1), dict(top_p=0.0),
                dict(top_p=1.5), dict(temperature=0.0), dict(temperature=float("nan")), dict(prefill=False)):
        with pytest.raises(ValueError):
            RunConfig(sample=True, **bad)
    RunConfig(top_p=7.0)  # the sampling fields are not read without sample


def test_sample_rejects_executor_factory():
    import torch
    from distributed_inference_demo_amd.serve import run_rank
    with pytest.raises(ValueError, match="executor_factory"):
        run_rank(RunConfig(sample=True, num_sample=1, max_length=2), 0, 1, torch.device("cpu"),
                 executor_factory=lambda *a, **k: None)


def test_request_seed_distinct_and_stable():
    seeds = [request_seed(0, i) for i in range(4096)] + [request_seed(1, i) for i in range(4096)]
    assert len(set(seeds)) == len(seeds) and all(0 <= s < 2 ** 64 for s in seeds)
    assert request_seed(0, 0) == 0x5E41AB087439611E and request_seed(0, 1) == 0x64684C4F0FD784B4
    assert request_seed(2 ** 64 + 5, 7) == request_seed(5, 7)
