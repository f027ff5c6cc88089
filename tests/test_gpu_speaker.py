"""GPU: SpeakerSLMFT / EmocaConverter (reference code/seq2seq_pretrain.py:516-842) on the HIP library against the CPU checker
of tests/speaker_ref.py (oracle.ref_cpu + stock torch.nn.LSTM / Linear) on the same seeded weights and inputs.  f32 parity mode
unless stated.  Tolerances: emoca 1e-4 (the VQ-decode tolerance), mesh 1e-4 * max(1, max|ref|), logits 2e-3, losses 1e-3
relative, decoded motion 1e-3 when every argmax is clear of 5e-3 (tests/test_gpu_slm.py)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

MESH = 363
SEED = 20260928


@pytest.fixture(scope="module")
def spk_sd():
    from dimx import weights
    return weights.synth_state_dict(weights.speaker_slmft_spec(MESH), SEED)


@pytest.fixture(scope="module")
def model():
    from dimx.seq2seq_pretrain import SpeakerSLMFT
    return SpeakerSLMFT(mesh_dim=MESH).cuda()


def _inputs(B, T, lens, seed=6, mesh=MESH):
    from dimx import prng
    templ = torch.from_numpy(prng.normal(seed, "spk.t", (B, mesh))) * 0.1
    v_s = templ[:, None] + 0.05 * torch.from_numpy(prng.normal(seed, "spk.v", (B, T, mesh)))
    v_e = torch.from_numpy(prng.normal(seed, "spk.e", (B, T, 56)))
    v_a = torch.from_numpy(prng.normal(seed, "spk.a", (B, T, 768)))
    mask = torch.zeros(B, T, dtype=torch.bool)
    for j, n in enumerate(lens):
        mask[j, :n] = True
    return v_s, v_e, v_a, mask, templ


@pytest.mark.parametrize("B,L", [(3, 26), (1, 299)])
def test_forward_vq_decoder_on_given_tokens(spk_sd, model, B, L):
    import speaker_ref
    from dimx import prng
    tokens = torch.from_numpy(prng.integers(3, "spk.tok", (B, L), 0, 512))
    mesh, emoca = model.forward_vq_decoder(tokens.cuda(), type="emoca", mode="val")
    ref_mesh, ref_emoca = speaker_ref.forward_vq_decoder(spk_sd, tokens)
    e_err = (emoca.cpu() - ref_emoca).abs().max().item()
    print("emoca err %.2e" % e_err)
    assert e_err < 1e-4, e_err
    # the head judged on identical input: the checker's own emoca
    eng = model.engine("cuda:0")
    scale = max(1.0, ref_mesh.abs().max().item())
    ref64 = speaker_ref.mesh_head(spk_sd, ref_emoca, dtype=torch.float64)
    own = (ref_mesh.double() - ref64).abs().max().item()
    for safe in (False, True):
        got = eng.mesh_head(ref_emoca.cuda(), None, safe=safe).cpu()
        err = (got - ref_mesh).abs().max().item()
        print("mesh head B=%d L=%d %s: err %.2e (tolerance %.2e, checker f32 vs f64 %.2e)"
              % (B, L, "safe" if safe else "group", err, 1e-4 * scale, own))
        assert err < 1e-4 * scale
    assert own * 10 < 1e-4 * scale, "the checker's own f32 noise %g is not 10x below the tolerance" % own
    assert tuple(mesh.shape) == (B, L, MESH) and torch.isfinite(mesh).all()
    assert eng.lstm_faults() == 0


@pytest.mark.parametrize("with_ids", [True, False])
def test_forward_train_matches_checker(spk_sd, with_ids):
    import speaker_ref
    from dimx.seq2seq_pretrain import SpeakerSLMFT
    B, T, lens = 3, 40, [40, 31, 17]
    v_s, v_e, v_a, mask, templ = _inputs(B, T, lens)
    ids = torch.tensor([2, 14, 7]) if with_ids else None
    ids_gpu = ids.cuda() if with_ids else None
    mouth = [0, 5, 17, 64, 120]
    m = SpeakerSLMFT(mesh_dim=MESH, mouth_map=mouth).cuda()
    total, d, pred, tok, mesh = m(v_s.cuda(), v_e.cuda(), v_a.cuda(), mask.cuda(), templ.cuda(), mode="train",
                                  speaker_ids=ids_gpu, return_tokens=True, return_mesh=True)
    rt, rd, rpred, aux = speaker_ref.speaker_forward(spk_sd, v_s, v_e, v_a, mask, templ, "train", ids, mouth_map=mouth)
    assert set(d) == {"l_ce_s", "l_ce_l", "l_cont_s", "l_cont_l", "nce", "c_acc"}
    assert d["l_ce_s"] == 0 and d["nce"] == 0 and d["c_acc"] == 0
    assert tuple(pred.shape) == (B, T - 1, 56) and tuple(mesh.shape) == (B, T - 1, MESH)
    x_l = torch.zeros(B, T, 384) if ids is None else spk_sd["speaker_embed.weight"][ids].unsqueeze(1).repeat(1, T, 1)
    l_ce, logits = m.forward_decoder(x_l.cuda(), aux["z"].cuda(), v_a.cuda(), mask.cuda(), mode="train")
    err = (logits.cpu() - aux["logits"]).abs().max().item()
    print("logits err %.2e, l_ce %.6f vs %.6f" % (err, float(d["l_ce_l"]), float(rd["l_ce_l"])))
    assert err < 2e-3
    assert abs(float(d["l_ce_l"]) - float(rd["l_ce_l"])) < 1e-3 * max(1.0, abs(float(rd["l_ce_l"])))
    top = aux["logits"].topk(2, -1).values
    if ((top[..., 0] - top[..., 1]) > 5e-3).all():
        assert torch.equal(tok.cpu(), aux["tokens"])
        assert (pred.cpu() - rpred).abs().max() < 1e-3
        assert abs(float(total) - float(rt)) < 1e-3 * abs(float(rt))
        assert abs(float(d["l_cont_l"]) - float(rd["l_cont_l"])) < 1e-3 * abs(float(rd["l_cont_l"]))
        assert abs(float(d["l_cont_s"]) - float(rd["l_cont_s"])) < 1e-3 * abs(float(rd["l_cont_s"]))
    # whatever the argmax decisions were: the continuous losses that follow from the tokens the engine chose
    from oracle import ref_cpu
    import torch.nn.functional as F
    e_tok = ref_cpu.vq_decode(spk_sd, tok.cpu().long(), "speaker_vq.")
    m_tok = speaker_ref.mesh_head(spk_sd, e_tok, templ)
    idx = torch.as_tensor(mouth)
    l_mouth = F.mse_loss(m_tok.view(B, T - 1, -1, 3)[:, :, idx], v_s[:, 1:].reshape(B, T - 1, -1, 3)[:, :, idx])
    l_emoca = F.mse_loss(e_tok, v_e[:, 1:])
    print("l_cont_s %.6e vs %.6e, l_cont_l %.6f vs %.6f" % (float(d["l_cont_s"]), float(l_mouth), float(d["l_cont_l"]), float(l_emoca)))
    assert abs(float(d["l_cont_s"]) - float(l_mouth)) < 1e-3 * abs(float(l_mouth))
    assert abs(float(d["l_cont_l"]) - float(l_emoca)) < 1e-3 * abs(float(l_emoca))
    assert abs(float(total) - float(d["l_ce_l"]) - float(d["l_cont_l"])) < 1e-5 * abs(float(total))
    # without a mouth map the head is not run and the entry is 0
    t2, d2, p2 = SpeakerSLMFT(mesh_dim=MESH).cuda()(v_s.cuda(), v_e.cuda(), v_a.cuda(), mask.cuda(), templ.cuda(), mode="train",
                                                    speaker_ids=ids_gpu)
    assert d2["l_cont_s"] == 0 and torch.equal(p2, pred)


@pytest.mark.parametrize("noisy", [False, True])
def test_forward_val_tokens_identical(spk_sd, model, noisy):
    import speaker_ref
    from dimx import prng
    B, T = 2, 40
    v_s, v_e, v_a, mask, templ = _inputs(B, T, [40, 29], seed=9)
    noise = torch.from_numpy(prng.exponential(9, "spk.noise", (T - 1, B, 512))) if noisy else None
    ids = torch.tensor([0, 11])
    total, d, pred, tok = model(v_s.cuda(), v_e.cuda(), v_a.cuda(), mask.cuda(), templ.cuda(), mode="val", speaker_ids=ids.cuda(),
                                noise=noise.cuda() if noisy else None, greedy=not noisy, return_tokens=True)
    rt, rd, rpred, aux = speaker_ref.speaker_forward(spk_sd, v_s, v_e, v_a, mask, templ, "val", ids, noise=noise)
    assert tuple(tok.shape) == (B, T - 1)
    assert torch.equal(tok.cpu(), aux["tokens"]), "generated code indices differ from the checker's"
    assert (pred.cpu() - rpred).abs().max() < 1e-4
    assert d["l_ce_l"] == 0.0 and abs(float(total) - float(rt)) < 1e-3 * abs(float(rt))


def test_emoca_converter_matches_checker():
    import speaker_ref
    from dimx import prng, weights
    from dimx.seq2seq_pretrain import EmocaConverter
    from oracle import ref_cpu
    B, T = 3, 30
    c = EmocaConverter(mesh_dim=MESH).cuda()
    sd = weights.synth_state_dict(weights.vq_spec(prefix="speaker_vq.") + weights.emoca_converter_spec(MESH), SEED)
    v = torch.from_numpy(prng.normal(12, "conv.v", (B, T, 56)))
    templ = torch.from_numpy(prng.normal(12, "conv.t", (B, MESH)))
    templ[1] += 5.0       # a template row added to the wrong clip would show
    out, none = c(None, templ.cuda(), v.cuda())
    ref, dec = speaker_ref.converter_forward(sd, templ, v)
    assert none is None and tuple(out.shape) == (B, T, MESH)
    scale = max(1.0, ref.abs().max().item())
    eng = c.engine("cuda:0")
    # the head on the checker's own decoder output ...
    got = eng.mesh_head(dec.cuda(), templ.cuda()).cpu()
    assert (got - ref).abs().max().item() < 1e-4 * scale
    no_t = eng.mesh_head(dec.cuda(), None).cpu()
    assert (got - no_t - templ[:, None]).abs().max().item() < 1e-5 * scale     # row b went to clip b, and only there
    # ... and the whole forward (the VQ codes in front of it are integers and must agree)
    idx = eng.vq_encode(0, v.cuda(), None, pe_mode=1)
    assert torch.equal(idx.cpu().long(), ref_cpu.vq_encode(sd, v, "speaker_vq."))
    assert (out.cpu() - ref).abs().max().item() < 2e-4 * scale


def test_full_size_head_and_guard():
    """mesh_dim 70110 (70110 % 4 = 2: no tile divides it), B = 1, T = 27: the mesh against the checker, and a guard region
    behind mesh_out stays untouched."""
    import speaker_ref
    from dimx import prng, weights
    from dimx.engine import Engine
    V, B, L = 70110, 1, 26
    spec = weights.emoca_converter_spec(V)
    sd = weights.synth_state_dict([e for e in spec if e[2] != "unused"], SEED)
    eng = Engine("cuda:0", variant="speaker", mesh_dim=V)
    eng.load_state_dict(sd)
    emoca = torch.from_numpy(prng.normal(2, "full.e", (B, L, 56)))
    templ = torch.from_numpy(prng.normal(2, "full.t", (B, V)))
    guard = 4096
    buf = torch.full((B * L * V + guard,), 12345.0, device="cuda:0")
    out = buf[:B * L * V].view(B, L, V)
    eng.mesh_head(emoca.cuda(), templ.cuda(), out=out)
    torch.cuda.synchronize()
    assert bool((buf[B * L * V:] == 12345.0).all()), "the head wrote past mesh_out"
    assert bool((out != 12345.0).all()), "an element of mesh_out was not written"
    ref = speaker_ref.mesh_head(sd, emoca, templ)
    scale = max(1.0, ref.abs().max().item())
    err = (out.cpu() - ref).abs().max().item()
    print("full-size head: err %.2e, tolerance %.2e" % (err, 1e-4 * scale))
    assert err < 1e-4 * scale
    assert eng.lstm_faults() == 0


def test_both_numeric_modes_finite():
    from dimx import lib
    from dimx.seq2seq_pretrain import SpeakerSLMFT
    B, T = 2, 32
    v_s, v_e, v_a, mask, templ = _inputs(B, T, [32, 20], seed=3)
    outs = []
    for mode in (lib.MODE_PARITY_F32, lib.MODE_PERF_BF16):
        m = SpeakerSLMFT(mesh_dim=MESH, mouth_map=[1, 2, 3], numeric_mode=mode).cuda()
        tokens = torch.arange(B * (T - 1)).view(B, T - 1) % 512
        mesh, emoca = m.forward_vq_decoder(tokens.cuda(), mode="val", template=templ.cuda())
        total, d, pred = m(v_s.cuda(), v_e.cuda(), v_a.cuda(), mask.cuda(), templ.cuda(), mode="train")
        assert torch.isfinite(total) and torch.isfinite(mesh).all() and torch.isfinite(pred).all()
        assert torch.isfinite(torch.as_tensor(d["l_cont_s"]))
        outs.append((emoca.cpu(), mesh.cpu()))
    dev_e = (outs[0][0] - outs[1][0]).abs().max().item()
    dev_m = (outs[0][1] - outs[1][1]).abs().max().item()
    print("perf mode vs f32 on given tokens: emoca %.3e, mesh %.3e" % (dev_e, dev_m))
    assert dev_e < 0.15


def test_head_keys_belong_to_a_handle_with_the_head(spk_sd):
    """dimx_missing_weights counts the 20 head tensors only for a handle created with mesh_dim; the tensors the reference's
    forward never applies are accepted and ignored by every handle; a head tensor is unknown to a handle without the head."""
    from dimx import lib
    from dimx.engine import Engine
    plain, head = Engine("cuda:0", variant="slm"), Engine("cuda:0", variant="speaker", mesh_dim=MESH)
    assert head.missing_weights() - plain.missing_weights() == 20
    head.load_state_dict(spk_sd)
    assert head.missing_weights() == 0
    ignored = ("vertice_mapping.", "squasher.", "vertice_map_reverse2.", "vertice_map_reverse_lstm_2.", "speaker_embed.")
    plain.load_state_dict({k: v for k, v in spk_sd.items() if k.startswith(ignored) or k == "W"})
    with pytest.raises(lib.DimxError):
        plain.load_state_dict({"vertice_map_reverse.0.bias": spk_sd["vertice_map_reverse.0.bias"]})
    with pytest.raises(lib.DimxError):
        plain.mesh_head(torch.zeros(1, 4, 56, device="cuda:0"))
