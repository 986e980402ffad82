"""Cases, references and comparison functions for the towers' embedding front end (patch extraction, the patch GEMM with
its positional rows, the class-token rows, ln_pre; token + positional embedding and the EOT rows of the text tower).
No tests here: tests/test_embed.py (CPU) checks that these references and comparisons see the indexing errors the
end-to-end encode_* rule lets through, tests/test_embed_gpu.py (-m gpu) runs the kernels against them through
clipmi_dbg_embed_image / clipmi_dbg_embed_text.

Everything takes and returns torch tensors on the device of its inputs, so the GPU tests compute the float64 references
there and the CPU test on the host. The references are plain torch in float64 (or exact integer / bit arithmetic)."""
import numpy as np
import torch

# ---- geometries -----------------------------------------------------------------------------------------------------------
# name: patch, res, width. np = (res / patch)^2 patches per image, L = np + 1 tokens, patch_k = 3 patch^2 rounded up to 64.
# np is 9, 16, 25, 25, 49: a 16-row MFMA fragment straddles an image boundary in every one of them.
GEOMS = {
    "G1": dict(patch=32, res=96, width=256),     # u8 strip path; f32 / bf16 vector path; LN-folded ln_pre (split output)
    "G2": dict(patch=16, res=64, width=128),     # strip path; ln_fold 0
    "G3": dict(patch=14, res=70, width=256),     # scalar path for all three types; zero columns 588..639
    "G4": dict(patch=8, res=40, width=128),      # u8 through the vector path (res % 16 != 0)
    "G5": dict(patch=32, res=224, width=768),    # ViT-B/32's own geometry
}
# batch sizes. G1: M = 9, 126, 135, 261 (skinny kernel, its last size, a 128-row tile + 7, a 256-row tile + 5);
# G3: M = 25, 125, 150, 275; G5: 320 is the one case where the product's rule itself picks the 256 x 256 kernel
# (62 row tiles x 3 = 186 tiles >= 0.72 x 256; the smallest such B is 319)
BATCHES = {"G1": (1, 14, 15, 29), "G2": (1, 9, 17), "G3": (1, 5, 6, 11), "G4": (1, 9, 17), "G5": (1, 2, 3, 320)}
EMBED = 128

F32, BF16, U8 = 0, 1, 2          # clipmi.h element types

# the kernel's f32 constants of CLIP's transform (vit_kernels.hpp)
MEAN = np.array([0.48145466, 0.4578275, 0.40821073], dtype=np.float32)
STD = np.array([0.26862954, 0.26130258, 0.27577711], dtype=np.float32)


def dims(name):
    g = GEOMS[name]
    grid = g["res"] // g["patch"]
    k = 3 * g["patch"] ** 2
    return dict(P=g["patch"], R=g["res"], W=g["width"], grid=grid, np=grid * grid, L=grid * grid + 1, k=k,
                patch_k=(k + 63) // 64 * 64)


def algos(name):
    """0 = the product's choice; 1 = the 128 x 128 kernel (N % 128 == 0, K % 64 == 0: every geometry); 2 = the
    256 x 256 kernel, which needs N % 256 == 0."""
    return (0, 1, 2) if GEOMS[name]["width"] % 256 == 0 else (0, 1)


# ---- state dicts, built by hand from shapes (weights.infer_dims reads shapes only) -------------------------------------------
def _block(sd, prefix, width):
    """One residual block. The embedding front end never reads it: zeros (ones for the LayerNorm weights) keep the
    packer's work and the blobs small."""
    p = f"{prefix}.resblocks.0"
    for ln in ("ln_1", "ln_2"):
        sd[f"{p}.{ln}.weight"] = torch.ones(width)
        sd[f"{p}.{ln}.bias"] = torch.zeros(width)
    for key, shape in (("attn.in_proj_weight", (3 * width, width)), ("attn.in_proj_bias", (3 * width,)),
                       ("attn.out_proj.weight", (width, width)), ("attn.out_proj.bias", (width,)),
                       ("mlp.c_fc.weight", (4 * width, width)), ("mlp.c_fc.bias", (4 * width,)),
                       ("mlp.c_proj.weight", (width, 4 * width)), ("mlp.c_proj.bias", (width,))):
        sd[f"{p}.{key}"] = torch.zeros(*shape)


def vision_state_dict(name, mode, seed=0):
    """mode "exact": conv1.weight integers in [-4, 4], class / positional embedding multiples of 1/8 in [-4, 4] - with
    integer pixels in [-8, 8] every partial sum of a row is an integer below 2^24 plus a multiple of 1/8, exact in f32
    in any order. mode "gauss": the scales of weights.random_state_dict (gain 1.5)."""
    d = dims(name)
    W, P, L = d["W"], d["P"], d["L"]
    g = torch.Generator(device="cpu")
    g.manual_seed(1000 + seed)
    sd = {}
    if mode == "exact":
        sd["visual.conv1.weight"] = torch.randint(-4, 5, (W, 3, P, P), generator=g).float()
        sd["visual.class_embedding"] = torch.randint(-32, 33, (W,), generator=g).float() / 8
        sd["visual.positional_embedding"] = torch.randint(-32, 33, (L, W), generator=g).float() / 8
    else:
        sd["visual.conv1.weight"] = torch.randn(W, 3, P, P, generator=g) * ((3 * P * P) ** -0.5 * 1.5)
        sd["visual.class_embedding"] = torch.randn(W, generator=g) * W ** -0.5
        sd["visual.positional_embedding"] = torch.randn(L, W, generator=g) * W ** -0.5
    sd["visual.ln_pre.weight"] = 1.0 + 0.1 * torch.randn(W, generator=g)
    sd["visual.ln_pre.bias"] = 0.1 * torch.randn(W, generator=g)
    _block(sd, "visual.transformer", W)
    sd["visual.ln_post.weight"] = torch.ones(W)
    sd["visual.ln_post.bias"] = torch.zeros(W)
    sd["visual.proj"] = torch.zeros(W, EMBED)
    # the text side: only what infer_dims reads
    sd["token_embedding.weight"] = torch.zeros(2, 64)
    sd["positional_embedding"] = torch.zeros(2, 64)
    sd["ln_final.weight"] = torch.ones(64)
    sd["text_projection"] = torch.zeros(64, EMBED)
    return sd


TEXT_TOWERS = {128: dict(ctx=16, vocab=512), 512: dict(ctx=77, vocab=600), 768: dict(ctx=77, vocab=600)}
TEXT_Q = (1, 3, 4, 5, 64, 65, 257)       # 257: the fused kernel's EOT block walks the prompts 256 at a time


def text_state_dict(width, seed=0):
    t = TEXT_TOWERS[width]
    g = torch.Generator(device="cpu")
    g.manual_seed(2000 + seed + width)
    sd = {}
    sd["token_embedding.weight"] = torch.randn(t["vocab"], width, generator=g) * 0.2
    sd["positional_embedding"] = torch.randn(t["ctx"], width, generator=g) * 0.1
    _block(sd, "transformer", width)
    sd["ln_final.weight"] = torch.ones(width)
    sd["ln_final.bias"] = torch.zeros(width)
    sd["text_projection"] = torch.zeros(width, EMBED)
    # the vision side: only what infer_dims reads
    sd["visual.conv1.weight"] = torch.zeros(64, 3, 2, 2)
    sd["visual.positional_embedding"] = torch.zeros(2, 64)
    return sd


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def exact_pixels(name, B, seed=0):
    """Integers in [-8, 8] as f32 [B][3][R][R] (exact in bf16 too)."""
    d = dims(name)
    g = torch.Generator(device="cpu")
    g.manual_seed(3000 + seed + B)
    return torch.randint(-8, 9, (B, 3, d["R"], d["R"]), generator=g, dtype=torch.int8).float()


def rounding_pixels(name, B, seed=0):
    """f32 values that bf16 has to ROUND: Gaussian data plus the awkward ones - exact ties to both sides, -0, a tiny value,
    large ones (all normal numbers: pixels are never subnormal)."""
    d = dims(name)
    g = torch.Generator(device="cpu")
    g.manual_seed(4000 + seed + B)
    x = torch.randn(B, 3, d["R"], d["R"], generator=g) * 1.3
    awkward = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8), -0.0, 0.0, 1e-30, -3.0e38, 65504.0,
                            1.0 + 2.0 ** -8 + 2.0 ** -23, 1.0 + 2.0 ** -8 - 2.0 ** -24])
    flat = x.reshape(-1)
    flat[:awkward.numel()] = awkward                    # the first row of image 0 ...
    flat[-awkward.numel():] = awkward                   # ... and the last row of the last one
    return x


def u8_pixels(name, B):
    """Image 0 is a ramp that shows all 256 byte values in every channel; every other image's byte is a hash of its own
    linear index (b, c, y, x), so a pixel fetched from anywhere else is almost surely another byte."""
    d = dims(name)
    R = d["R"]
    idx = torch.arange(B * 3 * R * R, dtype=torch.int64).reshape(B, 3, R, R)
    x = ((idx * 2654435761) >> 13) & 0xff
    c = torch.arange(3).reshape(3, 1, 1)
    x[0] = (torch.arange(R * R).reshape(1, R, R) + 37 * c) & 0xff
    return x.to(torch.uint8)


def text_ids(width, Q, seed=0):
    """int32 [Q][L]. Prompt q is of kind q % 6: 0 the maximum id at position 0; 1 at position L - 1; 2 the maximum id
    twice (the first one wins, as torch.argmax does); 3 all ids equal; 4 ids -1 and `vocab` (the documented clamp to 0
    and vocab - 1; `vocab` is also the row's maximum); 5 plain random ids."""
    t = TEXT_TOWERS[width]
    L, vocab = t["ctx"], t["vocab"]
    g = torch.Generator(device="cpu")
    g.manual_seed(5000 + seed + Q + width)
    ids = torch.randint(1, vocab - 2, (Q, L), generator=g, dtype=torch.int32)
    for q in range(Q):
        kind = q % 6
        if kind == 0:
            ids[q, 0] = vocab - 1
        elif kind == 1:
            ids[q, L - 1] = vocab - 1
        elif kind == 2:
            ids[q, 3] = vocab - 1
            ids[q, 9] = vocab - 1
        elif kind == 3:
            ids[q, :] = 7 + q % 5
        elif kind == 4:
            ids[q, 2] = -1
            ids[q, 5] = vocab
    return ids


# ---- references ----------------------------------------------------------------------------------------------------------
def bf16_rne(x64):
    """float64 -> bf16, one rounding to nearest even done here: m in [0.5, 1) times 2^8 is exact in float64, np.rint
    rounds halves to even. (torch's double -> bf16 rounds to f32 first.) Normal-range values only."""
    m, e = np.frexp(np.asarray(x64, dtype=np.float64))
    y = np.ldexp(np.rint(m * 256.0), e - 8)
    return torch.from_numpy(y.astype(np.float32)).to(torch.bfloat16)       # exact: y has 8 significant bits


def u8_table(mutation=None):
    """bf16 [3][256]: per (channel, byte) the bf16-RNE of the float64 value of (byte / 255 - mean_c) / std_c with the
    kernel's f32 constants."""
    byte = np.arange(256, dtype=np.float64)[None, :]
    mean = MEAN.astype(np.float64)[:, None]
    std = STD.astype(np.float64)[:, None].copy()
    if mutation == "blue_by_green_std":
        std[2] = std[1]
    return bf16_rne((byte / 255.0 - mean) / std)


def to_patches(x, name):
    """[B][3][R][R] -> [B*np][patch_k]: column c*P*P + py*P + px (conv1.weight flattened), +0 beyond 3 P^2."""
    d = dims(name)
    B, P, grid = x.shape[0], d["P"], d["grid"]
    p = x.reshape(B, 3, grid, P, grid, P).permute(0, 2, 4, 1, 3, 5).reshape(B * d["np"], d["k"])
    if d["patch_k"] != d["k"]:
        p = torch.cat([p, torch.zeros(p.shape[0], d["patch_k"] - d["k"], dtype=p.dtype, device=p.device)], dim=1)
    return p.contiguous()


PIXEL_MUTATIONS = ("last_column_zero", "last_row_tail_zero", "blue_by_green_std", "swap_patches_0_1")
ROW_MUTATIONS = ("no_pos_last_patch", "cls_zero", "pos_shifted")
MUTATIONS = PIXEL_MUTATIONS + ROW_MUTATIONS


def ref_patches(pixels, name, mutation=None):
    """The bf16 patch matrix the device must produce, bit for bit. pixels: f32 (rounded to bf16, nearest even), bf16 (moved)
    or uint8 (CLIP's transform tail through u8_table). `mutation`: what a kernel bug of that name would produce."""
    d = dims(name)
    x = pixels.clone()
    if mutation == "last_column_zero":
        x[..., -1] = 0
    elif mutation == "last_row_tail_zero":
        x[:, :, -1, -8:] = 0
    if x.dtype == torch.uint8:
        table = u8_table(mutation).to(x.device)
        c = torch.arange(3, device=x.device).reshape(1, 3, 1, 1).expand_as(x)
        v = table[c, x.long()]
    else:
        v = x.to(torch.bfloat16)
    p = to_patches(v, name)
    if mutation == "swap_patches_0_1":
        p = p.reshape(-1, d["np"], d["patch_k"]).clone()
        p[:, [0, 1]] = p[:, [1, 0]]
        p = p.reshape(-1, d["patch_k"])
    return p


def ref_rows(patches, sd, name, mutation=None):
    """float64 [B*L][W]: cat(class_embedding, patches . conv1.weight^T) + positional_embedding, on the bf16 patch matrix
    and the bf16-rounded conv weights (what the device multiplies)."""
    d = dims(name)
    dev = patches.device
    W, L, n = d["W"], d["L"], d["np"]
    w = sd["visual.conv1.weight"].reshape(W, d["k"]).to(torch.bfloat16).to(dev).double()
    cls = sd["visual.class_embedding"].to(dev).double()
    pos = sd["visual.positional_embedding"].to(dev).double()
    if mutation == "cls_zero":
        cls = torch.zeros_like(cls)
    B = patches.shape[0] // n
    conv = (patches[:, :d["k"]].double() @ w.t()).reshape(B, n, W)
    ppos = pos[1:]
    if mutation == "no_pos_last_patch":
        ppos = ppos.clone()
        ppos[-1] = 0
    elif mutation == "pos_shifted":
        ppos = pos[:-1]                         # patch p gets row p instead of row 1 + p
    rows = torch.cat([(cls + pos[0]).reshape(1, 1, W).expand(B, 1, W), conv + ppos], dim=1)
    return (rows + 0.0).reshape(B * L, W)        # + 0.0: a zero is +0, as the device's accumulator gives it


def ref_ln(rows, w, b):
    """float64 LayerNorm (eps 1e-5) of rows (any float type) with the f32 parameters w, b."""
    x = rows.double()
    mu = x.mean(dim=-1, keepdim=True)
    var = ((x - mu) ** 2).mean(dim=-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + 1e-5) * w.to(x.device).double() + b.to(x.device).double()


def ref_text_rows(sd, ids, mutation=None):
    """f32 [Q*L][W] = token_embedding[clamp(id, 0, vocab - 1)] + positional_embedding[t]: one f32 add per element."""
    tok, pos = sd["token_embedding.weight"].to(ids.device), sd["positional_embedding"].to(ids.device)
    Q, L = ids.shape
    if mutation == "pos_shifted":
        pos = torch.roll(pos, 1, dims=0)
    x = tok[ids.long().clamp(0, tok.shape[0] - 1)] + pos
    return x.reshape(Q * L, -1)


def ref_rowidx(ids):
    """int32 [Q]: q*L + the FIRST argmax of the raw ids (torch.argmax returns the first of equal maxima)."""
    Q, L = ids.shape
    return (torch.arange(Q, device=ids.device) * L + ids.argmax(dim=-1)).to(torch.int32)


# ---- comparisons: each returns (accepted, figure) ---------------------------------------------------------------------------
def _bits(t):
    t = t.contiguous()
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


def same_bits(got, want):
    """(every bit equal, number of elements that differ). NaN payloads and the sign of zero count."""
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    bad = int((_bits(got) != _bits(want)).sum().item())
    return bad == 0, bad


def rows_exact(got, ref64):
    """Exact mode: the f32 rows against the float64 reference, zero tolerance. The reference must itself be exactly
    representable (checked: a reference that f32 would round is a mistake in the case, not in the kernel)."""
    want = ref64.float()
    assert torch.equal(want.double(), ref64), "exact-mode reference is not representable in f32"
    return same_bits(got, want)


def rows_within(got, ref64, rel):
    """Tolerance mode: (max |got - ref| <= rel * max |ref| and everything finite, max |got - ref| / (rel * max |ref|))."""
    tol = rel * ref64.abs().max().item()
    if not torch.isfinite(got).all():
        return False, float("inf")
    err = (got.double() - ref64).abs().max().item()
    return err <= tol, err / tol


GEMM_REL = 2e-4      # f32 output of a bf16 GEMM with f32 accumulation over K <= 3072 (tests/test_kernels_gpu.py)
LN_REL = 2e-5        # f32 LayerNorm (tests/test_kernels_gpu.py test_layernorm)
