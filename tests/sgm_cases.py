"""Inputs shared by tools/make_goldens_sgm.py (which runs the reference SGM head / model_sgm_2 encoder) and the tests of
the drop-in: the alphabet of an 80-class converter, text lists, the seeded head parameters and visual tokens.  Both sides
rebuild them from seeds, so tests/golden/sgm.npz holds results only."""
import torch

# 79 symbols + the CTC blank = the 80 classes of the tiny model; with the four SGM tokens V = 84
ALPHABET = " !\"#&'()*+,-./0123456789:;?ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz"
assert len(ALPHABET) == 79 and len(set(ALPHABET)) == 79

# edge cases of make_context_batch: an empty line, lines shorter than S, exactly S, repeats, the longest line
CONTEXT_TEXTS = ["", "a", "ab", "hello", "A MOVE to stop", "aaaaaaa", "x" * 3 + "." + "y" * 9, ""]

# (B, L, N, D, d_txt, V, S) of the head cases: a small one (every gradient stored whole) and the real width
HEAD_CASES = {"small": (3, 23, 64, 64, 32, 20, 5), "d768": (2, 41, 256, 768, 256, 84, 5)}


class Converter:
    """the `character` attribute of the forks' CTCLabelConverter: the blank, then the alphabet"""

    def __init__(self, alphabet=ALPHABET):
        self.character = ['[blank]'] + list(alphabet)


def random_texts(B, L, V, seed, min_len=0):
    """B lines over the V - 5 symbols of vocab_for(V), the first exactly L characters long"""
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(min_len, L + 1, (B,), generator=g).tolist()
    lens[0] = L
    return ["".join(ALPHABET[int(i)] for i in torch.randint(0, V - 5, (n,), generator=g)) for n in lens]


def vocab_for(V):
    """stoi of a V-entry vocabulary: the converter of the first V - 5 symbols (+ blank) and the four tokens"""
    stoi = {ch: i for i, ch in enumerate(Converter(ALPHABET[:V - 5]).character)}
    for t in ("<pad>", "<eos>", "<bos_left>", "<bos_right>"):
        stoi[t] = len(stoi)
    return stoi


def perturb_head(head, seed):
    """seeded values for what the constructor leaves at ones / zeros (LayerNorm affine, Linear biases stay kaiming)"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in head.named_parameters():
            if "norm" in n:
                p.copy_((1.0 if n.endswith("weight") else 0.0) + 0.2 * torch.randn(p.shape, generator=g).to(p.dtype))


def vis_tokens(B, N, D, seed):
    """float32 visual tokens (the reference runs them in float64, exactly these values)"""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, N, D, generator=g) * 1.5 + 0.3


def head_inputs(case):
    """(head seed, texts, vis) of a HEAD_CASES entry"""
    B, L, N, D, dtx, V, S = HEAD_CASES[case]
    return 100 + L, random_texts(B, L, V, seed=L), vis_tokens(B, N, D, seed=N + D)
