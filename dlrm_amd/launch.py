"""Run the UNMODIFIED reference training script with the MI355X hot path swapped in.

    python -m dlrm_amd.launch --reference /path/to/facebookresearch/dlrm -- \
        --arch-sparse-feature-size=128 --arch-mlp-bot=13-512-256-128 --arch-mlp-top=1024-1024-512-256-1 \
        --arch-embedding-size=... --mini-batch-size=65536 --use-gpu ...
    torchrun --nproc-per-node 8 -m dlrm_amd.launch --reference ... -- ... --dist-backend=nccl --use-gpu

`run()` in the reference resolves `DLRM_Net` and `ext_dist` by module-global name at call time
(dlrm_s_pytorch.py:1076,1285,1329-1336), so the swap is two assignments: the reference keeps its CLI, data
generation, training loop, timing and printing; every device operation under `dlrm(...)`, `loss_fn`, `backward()`
and `optimizer.step()` runs in libdlrm_hip.so.  (INTEGRATION.md has the details and the raw ctypes binding.)
"""
from __future__ import annotations

import argparse
import importlib
import os
import sys
import types


def _stub_tensorboard_if_missing() -> None:
    """dlrm_s_pytorch.py:101 imports SummaryWriter unconditionally; provide a no-op when tensorboard is absent."""
    try:
        importlib.import_module("torch.utils.tensorboard")
        return
    except Exception:
        pass
    tb = types.ModuleType("torch.utils.tensorboard")

    class SummaryWriter:  # noqa: D401 - no-op stand-in
        def __init__(self, *a, **k): pass
        def add_scalar(self, *a, **k): pass
        def close(self): pass
    tb.SummaryWriter = SummaryWriter
    sys.modules["torch.utils.tensorboard"] = tb


def _wrap_quantize_dynamic() -> None:
    """--quantize-mlp-with-bit 8 | 16: run() calls `torch.quantization.quantize_dynamic(dlrm, {torch.nn.Linear}, qint8 | float16)`
    (dlrm_s_pytorch.py:1473-1480), which would swap the towers' layers for torch's CPU-only modules.  A dlrm_amd.DLRM_Net is answered with
    its own quantize_mlp (the same model comes back); everything else goes to torch's function unchanged.  Wrapped once."""
    import torch
    import dlrm_amd

    q = torch.quantization
    inner = q.quantize_dynamic
    if getattr(inner, "_dlrm_amd_wrapped", False):
        return

    def quantize_dynamic(model, qconfig_spec=None, dtype=torch.qint8, *args, **kwargs):
        if isinstance(model, dlrm_amd.DLRM_Net):
            model.quantize_mlp(8 if dtype is torch.qint8 else 16)
            return model
        return inner(model, qconfig_spec, dtype, *args, **kwargs)

    quantize_dynamic._dlrm_amd_wrapped = True
    quantize_dynamic._dlrm_amd_inner = inner
    q.quantize_dynamic = quantize_dynamic


def load_reference(reference_dir: str, device_tables: bool = False):
    """Import the reference's dlrm_s_pytorch with DLRM_Net / ext_dist replaced; returns the module."""
    import dlrm_amd
    from dlrm_amd import ext_dist

    if not any(os.path.isfile(os.path.join(reference_dir, "dlrm_s_pytorch" + ext)) for ext in (".py", ".pyc")):
        # (.pyc: a checkout compiled into a sourceless tree with py_compile)
        sys.exit("ERROR: %s does not contain dlrm_s_pytorch.py" % reference_dir)
    _stub_tensorboard_if_missing()
    if reference_dir not in sys.path:
        sys.path.insert(0, reference_dir)
    # the reference's own `import extend_distributed as ext_dist` must bind OUR implementation, so that the rank /
    # size globals DLRM_Net reads (dlrm_s_pytorch.py:252,353,518) and the ones run() sets are the same objects
    sys.modules["extend_distributed"] = ext_dist
    ref = importlib.import_module("dlrm_s_pytorch")
    ref.DLRM_Net = dlrm_amd.DLRM_Net
    ref.ext_dist = ext_dist
    _wrap_quantize_dynamic()
    if device_tables:
        import torch
        dev = torch.device("cuda", max(int(os.environ.get("LOCAL_RANK", "0")), 0))
        dlrm_amd.set_embedding_init(dev)
    return ref


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m dlrm_amd.launch")
    ap.add_argument("--reference", default=os.environ.get("DLRM_REFERENCE", "."),
                    help="checkout of facebookresearch/dlrm (directory holding dlrm_s_pytorch.py)")
    ap.add_argument("--device-tables", action="store_true",
                    help="allocate + initialise embedding tables directly in HBM (needed for Criteo-Terabyte sizes: the "
                         "reference's numpy float64 temporary does not fit host RAM); same distribution, torch RNG")
    ap.add_argument("--bf16-tables", choices=("stochastic", "nearest"), default=None,
                    help="store the embedding tables in bfloat16 (dlrm_amd.set_embedding_dtype): half the table bytes; the fused sparse "
                         "update rounds each touched row once per step, stochastically (reproducible: --bf16-seed) or to nearest; the rows can "
                         "be fetched inside the interaction kernels: --bf16-fuse-interact (and --narrow-fuse-interact at widths 16 / 32 / 64)")
    ap.add_argument("--bf16-seed", type=int, default=0, help="seed of the stochastic rounding of --bf16-tables")
    ap.add_argument("--bf16-fuse-interact", action="store_true",
                    help="with --bf16-tables: fetch the bfloat16 rows inside the interaction kernels, forward and backward "
                         "(DLRM_Net.fuse_bf16_interact; same bits as the default two-kernel form, no pooled [B, T*D] buffer); "
                         "--arch-sparse-feature-size 128, or 16 / 32 / 64 together with --narrow-fuse-interact")
    ap.add_argument("--qr-fuse-interact", action="store_true",
                    help="with the reference's --qr-flag: fetch and compose the quotient / remainder rows inside the interaction kernels, "
                         "forward and backward (DLRM_Net.fuse_qr_interact; same bits as the default two-kernel form, no pooled [B, T*D] "
                         "buffer and no pooled sums kept for the backward); --arch-sparse-feature-size 128, or 16 / 32 / 64 together with "
                         "--narrow-fuse-interact")
    ap.add_argument("--narrow-fuse-interact", action="store_true",
                    help="plain fp32 tables of --arch-sparse-feature-size 16 / 32 / 64: fetch the rows inside the interaction kernels, forward "
                         "and backward (DLRM_Net.fuse_narrow_interact; same bits as the default two-kernel form, no pooled [B, T*D] buffer).  "
                         "Together with --bf16-tables --bf16-fuse-interact the same for bfloat16 tables of those widths; with the reference's "
                         "--quantize-emb-with-bit 4|8 --inference-only the fused forward over the packed tables of those widths; with the "
                         "reference's --qr-flag and --qr-fuse-interact the same for quotient-remainder tables of those widths")
    ap.add_argument("--fused-adagrad", action="store_true",
                    help="with the reference's --optimizer=adagrad: update the embedding tables with the fused exact Adagrad kernel on "
                         "torch.optim.Adagrad's own state (DLRM_Net.fused_adagrad; no sparse COO gradient, the dense parameters stay with "
                         "torch's step); not built for bfloat16, QR or mixed-dimension tables")
    return ap


def main(argv=None) -> None:
    argv = list(sys.argv[1:] if argv is None else argv)
    ref_args = []
    if "--" in argv:
        i = argv.index("--")
        argv, ref_args = argv[:i], argv[i + 1:]
    a = build_parser().parse_args(argv)
    ref = load_reference(os.path.abspath(a.reference), a.device_tables)
    if a.bf16_tables is not None:
        import torch
        import dlrm_amd
        dlrm_amd.set_embedding_dtype(torch.bfloat16, a.bf16_tables, a.bf16_seed)
    if a.bf16_fuse_interact:
        if a.bf16_tables is None:
            sys.exit("ERROR: --bf16-fuse-interact needs --bf16-tables")
        import dlrm_amd
        dlrm_amd.DLRM_Net.fuse_bf16_interact = True        # every model run() builds from here on
    if a.qr_fuse_interact:
        import dlrm_amd
        dlrm_amd.DLRM_Net.fuse_qr_interact = True          # every model run() builds from here on (a model without QR tables ignores it)
    if a.narrow_fuse_interact:
        import dlrm_amd
        dlrm_amd.DLRM_Net.fuse_narrow_interact = True      # every model run() builds from here on (other widths ignore it)
    if a.fused_adagrad:
        import dlrm_amd
        dlrm_amd.DLRM_Net.fused_adagrad = True             # every model run() builds from here on (other optimizers ignore it)
    sys.argv = [os.path.join(a.reference, "dlrm_s_pytorch.py")] + ref_args
    ref.run()


if __name__ == "__main__":
    main()
