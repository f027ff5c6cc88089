"""CPU: the prompted oracle of tests/prompt_ref.py against oracle.ref_cpu.ar_generate, and the host side of
``prompt_frames`` (prompt lengths and the prefilled prefix from a mask, argument checks)."""
import pytest
import torch

torch.set_grad_enabled(False)
B, T, LENS = 3, 40, [40, 33, 7]


def _case(B, T, lens, seed=9):
    from dimx import prng
    v_s = torch.from_numpy(prng.normal(seed, "s2s.vs", (B, T, 56)))
    v_a = torch.from_numpy(prng.normal(seed, "s2s.va", (B, T, 768)))
    z = torch.from_numpy(prng.integers(seed, "s2s.z", (B, T), 0, 512))
    mask = torch.zeros(B, T, dtype=torch.bool)
    for j, n in enumerate(lens):
        mask[j, :n] = True
    z = torch.where(mask, z, torch.full_like(z, -100))
    return v_s, v_a, z, mask


@pytest.fixture(scope="module")
def case(full_sd):
    import prompt_ref
    from dimx import prng
    from oracle import ref_cpu
    v_s, v_a, z, mask = _case(B, T, LENS)
    ctx = prompt_ref.case_context(full_sd, v_s, v_a, mask)
    noise = torch.from_numpy(prng.exponential(11, "s2s.noise", (T - 1, B, 512)))
    free = {noisy: ref_cpu.ar_generate(full_sd, z[:, 0], T - 1, ctx, mask, noise if noisy else None, return_logits=True)
            for noisy in (False, True)}
    return dict(z=z, mask=mask, ctx=ctx, noise=noise, free=free)


@pytest.mark.parametrize("noisy", [False, True])
def test_one_token_prompt_is_ar_generate(full_sd, case, noisy):
    import prompt_ref
    tok, lg = prompt_ref.prompted_generate(full_sd, case["z"][:, :1], [1, 1, 1], T - 1, case["ctx"], case["mask"],
                                           case["noise"] if noisy else None)
    ref_tok, ref_lg = case["free"][noisy]
    assert torch.equal(tok, ref_tok) and torch.equal(lg, ref_lg)
    # lengths are honoured, not the prompt's width: a wider prompt of other codes with plen = 1 changes nothing
    tok2, _ = prompt_ref.prompted_generate(full_sd, case["z"][:, :17], [1, 1, 1], T - 1, case["ctx"], case["mask"],
                                           case["noise"] if noisy else None)
    assert torch.equal(tok2, ref_tok)


@pytest.mark.parametrize("noisy", [False, True])
def test_continuation_reproduces_the_free_generation(full_sd, case, noisy):
    import prompt_ref
    ref_tok, ref_lg = case["free"][noisy]
    seq = torch.cat([case["z"][:, :1], ref_tok], 1)
    tok, lg = prompt_ref.prompted_generate(full_sd, seq[:, :17], [17, 9, 4], T - 1, case["ctx"], case["mask"],
                                           case["noise"] if noisy else None)
    assert torch.equal(tok, ref_tok) and torch.equal(lg, ref_lg)


def test_a_prompt_of_other_codes_changes_the_generation(full_sd, case):
    import prompt_ref
    plen = [17, 9, 4]
    tok, _ = prompt_ref.prompted_generate(full_sd, case["z"][:, :17], plen, T - 1, case["ctx"], case["mask"], None)
    free = case["free"][False][0]
    gen = torch.zeros_like(tok, dtype=torch.bool)
    for b, p in enumerate(plen):
        assert torch.equal(tok[b, :p - 1], case["z"][b, 1:p].clamp(min=0))
        gen[b, p - 1:] = True
    assert (tok != free)[gen].float().mean() > 0.5
    # negative prompt entries (clip 2 has 7 valid codes) count as token 0
    tok_all, _ = prompt_ref.prompted_generate(full_sd, case["z"][:, :17], None, T - 1, case["ctx"], case["mask"], None)
    assert bool((tok_all[2, 6:16] == 0).all())


def test_prompt_lengths_from_a_mask():
    from dimx.seq2seq_pretrain import prompt_lengths
    mask = torch.zeros(4, 40, dtype=torch.bool)
    lens = [40, 33, 7, 17]
    for j, n in enumerate(lens):
        mask[j, :n] = True
    plen, p0 = prompt_lengths(mask, 17, lens)
    assert plen.dtype == torch.int32 and plen.tolist() == [17, 17, 7, 17] and p0 == 7     # a clip shorter than prompt_frames
    plen, p0 = prompt_lengths(mask, 17)                                                  # no host lengths: one .item()
    assert plen.tolist() == [17, 17, 7, 17] and p0 == 7
    plen, p0 = prompt_lengths(mask, 5, lens)
    assert plen.tolist() == [5, 5, 5, 5] and p0 == 5
    mask[2] = False                                                                      # an empty clip still has the start token
    plen, p0 = prompt_lengths(mask, 17, [40, 33, 0, 17])
    assert plen.tolist() == [17, 17, 1, 17] and p0 == 1


def test_prompt_frames_must_leave_a_frame_to_generate():
    from dimx.seq2seq_pretrain import SLMFT
    m = SLMFT().eval()
    x = torch.zeros(2, 12, 56)
    a = torch.zeros(2, 12, 768)
    mask = torch.ones(2, 12, dtype=torch.bool)
    for bad in (12, 13, 0):
        with pytest.raises(ValueError):
            m(x, x, a, mask, mode="val", prompt_frames=bad)
        with pytest.raises(ValueError):
            m.forward_decoder(None, torch.zeros(2, 12, dtype=torch.long), a, mask, "val", v_speaker=x, prompt_frames=bad)
    with pytest.raises(ValueError):
        m(x, x, a, mask, mode="train", prompt_frames=5)
