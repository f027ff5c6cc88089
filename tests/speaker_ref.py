"""CPU checker for the DIM-Speaker parts (SpeakerSLMFT / EmocaConverter, reference code/seq2seq_pretrain.py:516-842): the
project's oracle (oracle.ref_cpu: VQ-VAE encode / decode, the SLM decoder with absolute positional embedding) composed with
stock torch.nn.LSTM / nn.Linear / F.leaky_relu loaded from the same state dict -- those torch modules ARE the reference's
arithmetic for the converter head."""
import torch
import torch.nn.functional as F

from oracle import ref_cpu

LSTM_PREFIX = "vertice_map_reverse_lstm."


def lstm_module(sd, dtype=torch.float32):
    m = torch.nn.LSTM(56, 384, 2, batch_first=True, bidirectional=True)
    m.load_state_dict({k[len(LSTM_PREFIX):]: v for k, v in sd.items() if k.startswith(LSTM_PREFIX)})
    return m.to(dtype).eval()


def mesh_head(sd, emoca, template=None, dtype=torch.float32):
    """vertice_map_reverse(vertice_map_reverse_lstm(emoca)[0]) (+ template[:, None]) -> [B,L,V]."""
    with torch.no_grad():
        y, _ = lstm_module(sd, dtype)(emoca.to(dtype))
        y = F.leaky_relu(F.linear(y, sd["vertice_map_reverse.0.weight"].to(dtype), sd["vertice_map_reverse.0.bias"].to(dtype)), 0.2)
        y = F.linear(y, sd["vertice_map_reverse.2.weight"].to(dtype), sd["vertice_map_reverse.2.bias"].to(dtype))
        if template is not None:
            y = y + template.to(dtype).unsqueeze(1)
    return y


def forward_vq_decoder(sd, tokens, template=None):
    """SpeakerSLMFT.forward_vq_decoder on code indices -> (mesh, emoca): SPEAKER VQ-VAE codebook + decoder, then the head."""
    emoca = ref_cpu.vq_decode(sd, tokens, "speaker_vq.")
    return mesh_head(sd, emoca, template), emoca


def context(sd, B, T, v_audio, speaker_ids=None):
    if speaker_ids is None:
        x_l = torch.zeros(B, T, 384)
    else:
        x_l = sd["speaker_embed.weight"][speaker_ids.long()].unsqueeze(1).repeat(1, T, 1)
    return torch.cat([x_l + sd["patch_embed_dec_l"], v_audio], dim=-1)


def encode_emoca(sd, v_speaker_emoca, mask):
    """z_s_emoca of SpeakerSLMFT.forward_vq: per-clip LISTENER VQ-VAE codes of the EMOCA stream, padded with -100."""
    B, T, _ = v_speaker_emoca.shape
    zs = []
    for i in range(B):
        z = ref_cpu.vq_encode(sd, v_speaker_emoca[i][mask[i]].unsqueeze(0), "listener_vq.")[0]
        zs.append(F.pad(z, (0, T - z.shape[-1]), value=-100))
    return torch.stack(zs, 0)


def speaker_forward(sd, v_speaker, v_speaker_emoca, v_audio, mask, template, mode="train", speaker_ids=None, noise=None,
                    mouth_map=None):
    """SpeakerSLMFT.forward (reference :708-757) -> (total, d, pred_emoca, aux)."""
    B, T = mask.shape
    z = encode_emoca(sd, v_speaker_emoca, mask)
    ctx = context(sd, B, T, v_audio, speaker_ids)
    if mode == "train":
        l_ce, logits = ref_cpu.slm_decoder_tf(sd, z, ctx, mask)
        tokens = logits.argmax(-1)
    else:
        l_ce, logits = 0.0, None
        tokens = ref_cpu.legacy_generate(sd, z[:, 0], T - 1, ctx, mask, noise=noise, temperature=1.0 if noise is not None else 0.0,
                                         prefix="decoder_joint.net.", depth=4, heads=12)
    emoca = ref_cpu.vq_decode(sd, tokens, "speaker_vq.")
    l_emoca = F.mse_loss(emoca, v_speaker_emoca[:, 1:])
    l_mouth, mesh = 0, None
    if mouth_map is not None:
        mesh = mesh_head(sd, emoca, template)
        idx = torch.as_tensor(mouth_map, dtype=torch.long)
        l_mouth = F.mse_loss(mesh.view(B, T - 1, -1, 3)[:, :, idx], v_speaker[:, 1:].reshape(B, T - 1, -1, 3)[:, :, idx])
    d = {"l_ce_s": 0, "l_ce_l": l_ce, "l_cont_s": l_mouth, "l_cont_l": l_emoca, "nce": 0, "c_acc": 0}
    return l_ce + l_emoca, d, emoca, {"logits": logits, "tokens": tokens, "z": z, "mesh": mesh}


def converter_forward(sd, template, v_speaker):
    """EmocaConverter.forward (reference :827-842): speaker_vq full forward (batched positional rows) -> head -> + template."""
    idx = ref_cpu.vq_encode(sd, v_speaker, "speaker_vq.")
    dec = ref_cpu.vq_decode(sd, idx, "speaker_vq.")
    return mesh_head(sd, dec, template), dec
