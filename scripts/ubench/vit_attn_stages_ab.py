"""Output bytes and launch times of the ViT attention entry points between LIBRARIES, in one process (every library opened with ctypes.CDLL).

    python scripts/ubench/vit_attn_stages_ab.py bytes LIB_A LIB_B          # every output array byte-equal, or exit 1
    python scripts/ubench/vit_attn_stages_ab.py time  LIB_A LIB_B [LIB_C]  # LIB_C: e.g. a copy of LIB_A, the control pair

`bytes` runs unopose_vit_attention (bf16), _f32, _f32_split and _f32_ss on seeded inputs at (B, H) = (3, 3) and (1, 12) -- B H is no multiple of 8,
so the padding workgroups past the last (image, head) run too -- and T = 1, 33, 261 (route 0), 545 (route 1), 1025, 1374 (route 2); the output
buffers are filled with a pattern before every launch.  `time` measures the workload's shapes, 64 x 12 x 1374 and 32 x 12 x 261, for
unopose_vit_attention and unopose_vit_attention_f32_ss: device events around 50 launches after 10 warm-up launches, the libraries in turn, seven
rounds; it prints every figure and each library's range."""
import ctypes
import hashlib
import sys

import torch

VP, I = ctypes.c_void_p, ctypes.c_int
ENTRY = ("unopose_vit_attention", "unopose_vit_attention_f32", "unopose_vit_attention_f32_split", "unopose_vit_attention_f32_ss")


def load(path):
    L = ctypes.CDLL(path)
    for name in ENTRY:
        getattr(L, name).argtypes = [VP, I, I, I, VP, VP]
        getattr(L, name).restype = I
    L.unopose_vit_attention_route.argtypes = [I, I]
    L.unopose_last_error.restype = ctypes.c_char_p
    return L


def split_layout(x):  # (..., C) fp32 -> (..., C / 32, 64) bf16: per 32-channel block [hi (32) | lo (32)]
    hi = x.bfloat16()
    lo = (x - hi.float()).bfloat16()
    blk = x.shape[:-1] + (x.shape[-1] // 32, 32)
    return torch.cat([hi.reshape(blk), lo.reshape(blk)], dim=-1).contiguous()


def inputs(B, T, H, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(B, T, 3 * H * 64, generator=g, device="cuda") * 1.5
    return {"bf16": x.bfloat16().contiguous(), "f32": x.contiguous(), "split": split_layout(x)}


def outputs(B, T, H):  # entry point -> (input kind, output buffer)
    C = H * 64
    return {"unopose_vit_attention": ("bf16", torch.empty(B, T, C, dtype=torch.bfloat16, device="cuda")),
            "unopose_vit_attention_f32": ("f32", torch.empty(B, T, C, dtype=torch.float32, device="cuda")),
            "unopose_vit_attention_f32_split": ("f32", torch.empty(B, T, C // 32, 64, dtype=torch.bfloat16, device="cuda")),
            "unopose_vit_attention_f32_ss": ("split", torch.empty(B, T, C // 32, 64, dtype=torch.bfloat16, device="cuda"))}


def launch(L, name, x, B, T, H, out):
    rc = getattr(L, name)(x.data_ptr(), B, T, H, out.data_ptr(), None)
    assert rc == 0, (name, rc, L.unopose_last_error())


def main():
    mode, paths = sys.argv[1], sys.argv[2:]
    libs = [load(p) for p in paths]
    for p in paths:
        print("library:", p, "sha256", hashlib.sha256(open(p, "rb").read()).hexdigest()[:16], flush=True)
    if mode == "bytes":
        bad = 0
        for B, H in ((3, 3), (1, 12)):
            for T in (1, 33, 261, 545, 1025, 1374):
                x = inputs(B, T, H, 1000 * B + T)
                for name, (kind, out) in outputs(B, T, H).items():
                    got = []
                    for L in libs:
                        out.view(torch.uint8).fill_(0x5A)
                        launch(L, name, x[kind], B, T, H, out)
                        torch.cuda.synchronize()
                        got.append(out.view(torch.uint8).cpu().clone())
                    eq = all(torch.equal(got[0], g) for g in got[1:])
                    sane = bool(torch.isfinite(out.float()).all())
                    bad += not (eq and sane)
                    print(f"({B},{H},{T:4d}) route {libs[0].unopose_vit_attention_route(T, H)} {name:34s} "
                          f"{'equal (bitwise)' if eq else 'DIFFERENT'}{'' if sane else ' NOT FINITE'}  sha256 "
                          f"{hashlib.sha256(got[0].numpy().tobytes()).hexdigest()[:16]}", flush=True)
        print("BITS: IDENTICAL" if not bad else f"BITS: {bad} arrays differ")
        sys.exit(1 if bad else 0)
    tags = ["A", "B", "C"][:len(libs)]
    for B, T, H in ((64, 1374, 12), (32, 261, 12)):
        x = inputs(B, T, H, T)
        outs = outputs(B, T, H)
        for name in ("unopose_vit_attention", "unopose_vit_attention_f32_ss"):
            kind, out = outs[name]
            us = {t: [] for t in tags}
            for rnd in range(7):
                for t, L in zip(tags, libs):
                    for _ in range(10):
                        launch(L, name, x[kind], B, T, H, out)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(50):
                        launch(L, name, x[kind], B, T, H, out)
                    e1.record()
                    torch.cuda.synchronize()
                    us[t].append(e0.elapsed_time(e1) * 1000.0 / 50)
            print(f"{name} {B}x{H}x{T}  " + "   ".join(f"{t} {min(v):9.2f} .. {max(v):9.2f} us" for t, v in us.items()))
            print("      " + " | ".join(f"{t} " + " ".join(f"{u:.2f}" for u in v) for t, v in us.items()), flush=True)


if __name__ == "__main__":
    main()
