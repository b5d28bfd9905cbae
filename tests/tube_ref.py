"""Test-only restatement of the tube model, its losses and its optimiser (deep_tube_learning/models.py, losses.py,
train_tube.py), in torch at any dtype, to check the HIP tube trainer against."""
import torch

ACT = {"relu": lambda beta: torch.nn.ReLU(), "softplus": lambda beta: torch.nn.Softplus(beta=beta),
       "tanh": lambda beta: torch.nn.Tanh(), "elu": lambda beta: torch.nn.ELU()}


class MLP(torch.nn.Module):
    """Linear, activation, repeated num_layers times, then a final Linear; state-dict keys layers.{0,2,...}.weight / .bias."""

    def __init__(self, input_dim, output_dim, num_units, num_layers, activation="relu", softplus_beta=1.0):
        super().__init__()
        act = ACT[activation](softplus_beta)
        self.layers = torch.nn.ModuleList([torch.nn.Linear(input_dim, num_units), act])
        for _ in range(num_layers - 1):
            self.layers.append(torch.nn.Linear(num_units, num_units))
            self.layers.append(act)
        self.layers.append(torch.nn.Linear(num_units, output_dim))

    def forward(self, x):
        for layer in self.layers:
            x = layer(x)
        return x


def pinball(fw, w, alpha):
    r = w - fw
    return torch.where(r > 0, alpha * r, (1 - alpha) * r.abs())


def loss(name, fw, w, alpha=0.8, delta=1.0):
    """scalar / scalar_horizon: Huber(delta) of the pinball residual, mean over every element; vector: pinball residuals summed
    per row, then Huber, mean over rows; error: MSE."""
    if name in ("scalar", "scalar_horizon"):
        l = pinball(fw, w, alpha)
        return torch.nn.functional.huber_loss(l, torch.zeros_like(l), delta=delta)
    if name == "vector":
        l = pinball(fw, w, alpha).sum(dim=-1)
        return torch.nn.functional.huber_loss(l, torch.zeros_like(l), delta=delta)
    if name == "error":
        return torch.nn.functional.mse_loss(fw, w)
    raise ValueError(name)


def eval_metrics(name, fw, w, alpha=0.8, delta=1.0):
    """evaluate_scalar_tube's metrics: loss, fraction of outputs with fw > w, mean |w - fw| over those."""
    m = fw > w
    return [float(loss(name, fw, w, alpha, delta)), float(m.double().mean()), float((w[m] - fw[m]).abs().mean())]


def optimizer(model, lr, gamma, step_size):
    """torch.optim.Adam (defaults) + StepLR stepped after every batch, as train_tube.py does."""
    opt = torch.optim.Adam(model.parameters(), lr=lr, foreach=False)
    return opt, torch.optim.lr_scheduler.StepLR(opt, step_size=step_size, gamma=gamma)
