"""Host side of the device-resident generator (ggad_amd/rng.py): the numpy restatement of `torch.randn` (tests/mt_randn_ref.py)
against torch itself, the number of words a draw consumes, the parse / format pair of `torch.get_rng_state()`, and the scripts' flag.
No GPU."""
import sys

import numpy as np
import pytest
import torch

import mt_randn_ref as R

SEEDS = (0, 5, 72)
SIZES = (16, 17, 31, 32, 300, 623, 624, 625, 71400, 71401)
BOUND = 5e-7      # absolute: about twice the 2.4e-7 measured between the restatement and torch (two float32 steps at |x| < 4); a wrong
#                   pairing or a wrong word count shows up as errors of order 1


@pytest.fixture(autouse=True)
def _keep_host_stream():
    st = torch.get_rng_state()
    yield
    torch.set_rng_state(st)


def _state_after(seed, prior):
    torch.manual_seed(seed)
    if prior:
        torch.randn(prior)
    return torch.get_rng_state()


def test_state_layout_of_the_cpu_generator():
    """Fact 4 of the design note: left / next after a fresh seed and after 116 words; seeded flag; 5,056 bytes."""
    from ggad_amd import rng
    torch.manual_seed(3)
    st = torch.get_rng_state()
    assert st.dtype == torch.uint8 and st.numel() == rng.STATE_BYTES == 5056
    q = st.numpy().view(np.uint64)
    assert int(q[0]) == 3 and int(q[1] & np.uint64(0xFFFFFFFF)) == 1 and int(q[1] >> np.uint64(32)) == 1 and int(q[2]) == 0
    assert rng.parse_rng_state(st)[1] == 624                 # a fresh generator regenerates its block before the first word
    torch.randn(100)                                         # 100 words, then 16 more: 100 % 16 != 0
    q = torch.get_rng_state().numpy().view(np.uint64)
    assert int(q[2]) == 116 and int(q[1] & np.uint64(0xFFFFFFFF)) == 509
    assert rng.parse_rng_state(torch.get_rng_state())[1] == 116


@pytest.mark.parametrize("prior", [0, 100])
@pytest.mark.parametrize("seed", SEEDS)
def test_restatement_equals_torch_randn(seed, prior):
    from ggad_amd import rng
    worst = 0.0
    for n in SIZES:
        words, pos = rng.parse_rng_state(_state_after(seed, prior))
        want = torch.randn(n).numpy()
        got, _, _ = R.randn(words, pos, n)
        assert got.dtype == np.float32 and got.shape == want.shape
        err = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
        worst = max(worst, err)
        assert err <= BOUND, (seed, prior, n, err)
    print(f"[restatement vs torch.randn] seed {seed} prior {prior}: max abs deviation {worst:.3e}")


@pytest.mark.parametrize("prior", [0, 100])
@pytest.mark.parametrize("seed", SEEDS)
def test_words_consumed_and_state_written_back(seed, prior):
    """After the restated draw, its state and position formatted back into the host generator make the next torch.randn(40) equal,
    bit for bit, to the one after the real torch.randn(n): pins `next`, `left` and the n + 16 rule.  The formatted state is also
    byte-equal to torch's own."""
    from ggad_amd import rng
    for n in SIZES:
        st = _state_after(seed, prior)
        words, pos = rng.parse_rng_state(st)
        torch.randn(n)
        after = torch.get_rng_state()
        want = torch.randn(40)
        _, words2, pos2 = R.randn(words, pos, n)
        mine = rng.format_rng_state(st, words2, pos2)
        assert torch.equal(mine, after), (seed, prior, n)
        torch.set_rng_state(mine)
        assert torch.equal(torch.randn(40), want), (seed, prior, n)


def test_a_draw_that_ends_on_a_block_boundary_stays_lazy():
    """624 words from a fresh seed: torch leaves next = 624, left = 1 and regenerates at the NEXT word; so does the restatement."""
    from ggad_amd import rng
    st = _state_after(0, 0)
    words, pos = rng.parse_rng_state(st)
    torch.randn(624)
    after = torch.get_rng_state()
    _, w2, p2 = R.randn(words, pos, 624)
    assert p2 == 624 and torch.equal(rng.format_rng_state(st, w2, p2), after)


@pytest.mark.parametrize("prior", [0, 16, 100, 624, 700])
def test_parse_then_format_is_the_identity(prior):
    from ggad_amd import rng
    st = _state_after(5, prior)
    words, pos = rng.parse_rng_state(st)
    assert words.dtype == np.uint32 and words.shape == (624,) and 0 <= pos <= 624
    assert torch.equal(rng.format_rng_state(st, words, pos), st)


def test_parse_refuses_what_is_not_a_cpu_generator_state():
    from ggad_amd import rng
    with pytest.raises(ValueError):
        rng.parse_rng_state(torch.zeros(100, dtype=torch.uint8))
    st = _state_after(0, 100)
    bad = st.clone()
    bad.numpy().view(np.uint64)[2] = 7                       # next no longer matches left
    with pytest.raises(ValueError):
        rng.parse_rng_state(bad)
    with pytest.raises(ValueError):
        rng.format_rng_state(st, np.zeros(624, dtype=np.uint32), 625)


def test_buffer_refusals_need_no_device():
    from ggad_amd import rng
    with pytest.raises(ValueError):
        rng._check_buffer(torch.zeros(15))
    with pytest.raises(ValueError):
        rng._check_buffer(torch.zeros(32, dtype=torch.float64))
    with pytest.raises(ValueError):
        rng._check_buffer(torch.zeros(8, 8)[:, :4])
    assert rng._check_buffer(torch.zeros(4, 4)) == 16


def test_device_noise_flag_parses_and_defaults_to_off(monkeypatch):
    import aegis
    import gaan
    import run
    assert gaan.parse(["--dataset", "Amazon"]).device_noise is False
    assert gaan.parse(["--dataset", "Amazon", "--device_noise"]).device_noise is True
    assert aegis.parse(["--dataset", "reddit"]).device_noise is False
    assert aegis.parse(["--dataset", "reddit", "--device_noise"]).device_noise is True
    monkeypatch.setattr(sys, "argv", ["run.py", "--dataset", "reddit"])
    assert run.parse().device_noise is False
    monkeypatch.setattr(sys, "argv", ["run.py", "--dataset", "reddit", "--device_noise"])
    assert run.parse().device_noise is True
