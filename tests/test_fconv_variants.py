"""The non-default fconv instantiations, on hardware.

The RAFT_AMD_* dispatch switches are read once per process, so every knob
setting runs in ONE fresh child process (this file, run as a script): it
computes 1x1 / 3x3 / 1x5 / 5x1 convs and the two GRU epilogues and checks
them against F.conv2d on the bf16-rounded inputs and weights.

Shapes are the smallest that reach every branch of the staging:
  * B=2, H=11: not a multiple of the 2/4/8-row tiles; with 5x1 there is an
    interior row block and a border row block at top and bottom;
  * two inputs C1=44 | C2=64: the seam is no multiple of 8 (scalar seam
    gather) and the k-chunk at 32 straddles both tensors (that k-step is
    guarded while the other steps of an interior tile take the fast path);
  * Cin=108 is no multiple of 32 (weight k-tail), N=72 no multiple of 32
    (weight n-tail, epilogue guard); GRU: hd=32, xd=76;
  * W=40 (8/16/32-wide tiles) and W=300 (64/128-wide): at least one tile
    is fully interior, one touches each border, the last one is partial.
Tolerances: plain convs as test_fconv_matches_conv2d (0.05*max|ref|+0.05),
GRU outputs as test_fconv_gru_pair_matches_eager (0.08).
"""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOB_VARS = ("BIG_MIN", "TILE2D", "TILE11", "PIPE", "PIPE_BIG", "STEM",
             "TINYN2")
B, H, C1, C2, N = 2, 11, 44, 64, 72
HD, XD = 32, 76
WIDTHS = (40, 300)
SHAPES = ((1, 1), (3, 3), (1, 5), (5, 1))


def _pack(w):
    n, cin, kh, kw = w.shape
    return w.permute(2, 3, 0, 1).reshape(kh * kw, n, cin).contiguous() \
        .to(torch.bfloat16)


def _conv(x_nhwc, w, bias, kh, kw):
    """fp32 SAME conv of an NHWC tensor with bf16-rounded weights."""
    y = F.conv2d(x_nhwc.float().permute(0, 3, 1, 2),
                 w.to(torch.bfloat16).float(), bias,
                 padding=(kh // 2, kw // 2))
    return y.permute(0, 2, 3, 1)


def run_variants(alltaps, mtiles, dump=None):
    """Body of the child process. Returns the list of failures."""
    sys.path.insert(0, ROOT)
    from raft_amd.ops import require_hip
    hip = require_hip()
    dev = torch.device("cuda:0")
    torch.manual_seed(1234)
    bad, outs = [], {}

    def check(tag, got, ref, tol):
        err = (got.float() - ref).abs().max().item()
        print(f"{tag}: err {err:.4f} tol {tol:.4f}", flush=True)
        outs[tag] = got.cpu()
        if not err < tol:
            bad.append(f"{tag}: {err} >= {tol}")

    for W in WIDTHS:
        a = torch.randn(B, H, W, C1, device=dev).to(torch.bfloat16)
        b = torch.randn(B, H, W, C2, device=dev).to(torch.bfloat16)
        ab = torch.cat([a, b], dim=-1)
        for kh, kw in SHAPES:
            w = torch.randn(N, C1 + C2, kh, kw, device=dev) * 0.1
            bias = torch.randn(N, device=dev)
            out = hip.fconv_plain(a, b, _pack(w), bias, kh, kw, 1, None, 0,
                                  0, 0, alltaps, mtiles, 1, None)
            ref = F.relu(_conv(ab, w, bias, kh, kw))
            check(f"plain {kh}x{kw} W={W}", out, ref,
                  0.05 * ref.abs().max().item() + 0.05)
        h = (torch.randn(B, H, W, HD, device=dev) * 0.5).to(torch.bfloat16)
        x = (torch.randn(B, H, W, XD, device=dev) * 0.5).to(torch.bfloat16)
        hx = torch.cat([h, x], dim=-1)
        for kh, kw in ((1, 5), (5, 1)):
            wzr = torch.randn(2 * HD, HD + XD, kh, kw, device=dev) * 0.1
            bzr = torch.randn(2 * HD, device=dev)
            wq = torch.randn(HD, HD + XD, kh, kw, device=dev) * 0.1
            bq = torch.randn(HD, device=dev)
            z, rh = hip.fconv_gru_zr(h, x, _pack(wzr), bzr, kh, kw)
            zr = torch.sigmoid(_conv(hx, wzr, bzr, kh, kw))
            check(f"gru z {kh}x{kw} W={W}", z, zr[..., :HD], 0.08)
            check(f"gru rh {kh}x{kw} W={W}", rh, zr[..., HD:] * h.float(),
                  0.08)
            # candidate stage on the kernel's own (bf16) rh and z
            hn = hip.fconv_gru_q(rh, x, _pack(wq), bq, kh, kw, z, h)
            q = torch.tanh(_conv(torch.cat([rh, x], dim=-1), wq, bq, kh, kw))
            ref = (1.0 - z.float()) * h.float() + z.float() * q
            check(f"gru q {kh}x{kw} W={W}", hn, ref, 0.08)
    torch.cuda.synchronize()
    if dump:
        torch.save(outs, dump)
    return bad


def _cases():
    cases = [("defaults", {}, -1, -1)]
    for t in (0, 1, 2, 4, 5, 8, 9):
        cases.append((f"TILE2D={t}", {"TILE2D": t}, -1, -1))
    cases.append(("TILE11=0", {"TILE11": 0}, -1, -1))
    cases.append(("PIPE=0", {"PIPE": 0}, -1, -1))
    for at in (0, 1):
        for mt in (1, 2, 4):
            cases.append((f"1row-at{at}-mt{mt}", {"TILE2D": 0, "TILE11": 0},
                          at, mt))
    for pb in (0, 1):
        cases.append((f"big-PIPE_BIG={pb}", {"PIPE_BIG": pb}, -1, -2))
    return cases


CASES = _cases()


def child_command(knobs, alltaps, mtiles, extra=()):
    """(argv, env) of the child process of one knob setting."""
    env = {k: v for k, v in os.environ.items()
           if not (k.startswith("RAFT_AMD_") and k[9:] in KNOB_VARS)}
    for k, v in knobs.items():
        env["RAFT_AMD_" + k] = str(v)
    argv = [sys.executable]
    if sys.flags.no_user_site:
        argv.append("-s")
    argv += [os.path.abspath(__file__), str(alltaps), str(mtiles), *extra]
    return argv, env


@pytest.mark.gpu
@pytest.mark.parametrize("knobs,alltaps,mtiles",
                         [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_fconv_variant_matches_conv2d(knobs, alltaps, mtiles):
    argv, env = child_command(knobs, alltaps, mtiles)
    # one child, no retry: a fault, abort or hang fails the case as it is
    r = subprocess.run(argv, env=env, capture_output=True, text=True,
                       timeout=180)
    assert r.returncode == 0, \
        f"child exit {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"


@pytest.mark.gpu
@pytest.mark.parametrize("k", [3, 1])
def test_fconv_stride2_two_inputs_odd_channels(k):
    """Stride 2 (parity slabs, always the guarded path) over the same odd
    channel counts: seam gather, k-tail and n-tail under stride 2."""
    from raft_amd.models.layers import Conv2dTF
    from raft_amd.ops import require_hip
    dev = torch.device("cuda:0")
    torch.manual_seed(k)
    conv = Conv2dTF(C1 + C2, N, k, stride=2).to(dev)
    x = torch.randn(B, C1 + C2, 22, 40, device=dev).to(torch.bfloat16)
    w = conv.weight.detach().float()
    with torch.no_grad():
        conv.weight.copy_(w.to(torch.bfloat16).float())
        ref = conv(x.float())
    xp = x.permute(0, 2, 3, 1)
    out = require_hip().fconv_plain(
        xp[..., :C1].contiguous(), xp[..., C1:].contiguous(), _pack(w),
        conv.bias.detach().float().contiguous(), k, k, 0, None, 0, 0, 0,
        -1, -1, 2, None)
    got = out.float().permute(0, 3, 1, 2)
    assert got.shape == ref.shape
    err = (got - ref).abs().max().item()
    assert err < 0.05 * ref.abs().max().item() + 0.05, err


if __name__ == "__main__":
    dump = sys.argv[4] if len(sys.argv) > 4 and sys.argv[3] == "--dump" \
        else None
    failures = run_variants(int(sys.argv[1]), int(sys.argv[2]), dump)
    for f in failures:
        print("FAIL", f)
    sys.exit(1 if failures else 0)
