"""Variables of a test net away from their initial state, shared by the CPU and GPU tests (tests/test_option_matrix.py builds
plan-only nets with it, tests/test_gpu_lock_map.py::make_net and tests/test_gpu_option_matrix.py real ones)."""
import torch


def perturb_variables(net, seed, perturb="scale"):
    """heads that produce non-trivial logits / detections, and the pass-through layers away from their initial batch-norm
    state (gamma 1, beta 0, moving mean 0, variance 1 fold to scale ~1, shift 0, which any mix-up of the coefficients would
    survive): every channel its own scale, an eighth of them negative.  ``perturb="scale"`` moves gamma and the moving
    variance (shift stays 0), ``"all"`` also beta and the moving mean -- see tests/test_gpu_lock_map.py::make_net for which
    test wants which.  Works on a plan-only net too (the variables are the same tensors, on the CPU); the caller re-packs."""
    g = torch.Generator().manual_seed(7919 + seed)
    with torch.no_grad():
        for i in (59, 67, 75, net.score_layer):
            net.params["yolo/convolutional%d/weights" % i].mul_(6.0)
            b = net.params["yolo/convolutional%d/biases" % i]
            b.copy_((torch.randn(b.shape, generator=g) * 0.5).to(b.device))
        for l in net.layers:
            if l.passthru and l.kind != "lin":
                rnd = lambda: torch.rand(l.cout, generator=g)
                gamma = (0.6 + 0.8 * rnd()) * torch.where(rnd() < 0.125, -1.0, 1.0)
                leaves = [("gamma", gamma), ("moving_variance", 0.5 + rnd())]
                if perturb == "all":
                    leaves += [("beta", 0.3 * torch.randn(l.cout, generator=g)), ("moving_mean", 0.2 * torch.randn(l.cout, generator=g))]
                for leaf, val in leaves:
                    t = net.params["yolo/convolutional%d/BatchNorm/%s" % (l.idx, leaf)]
                    t.copy_(val.to(t.device))
