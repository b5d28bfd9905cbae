"""PyTorch fp32 restatement of rsl_rl v1.0.2's recurrent policy path -- RECALLED, not copied: rsl_rl is not installed here and
the reference tree does not contain it (the reference names the class and its keys at legged_robot_config.py:240-248,266 and
exports it at helpers.py:288-313).  Test infrastructure only.

* ``Memory``: one ``nn.LSTM`` (gate order i, f, g, o; biases b_ih and b_hh).  Inference mode (no masks) feeds one step and keeps
  ``hidden_states``; batch mode (masks) runs padded trajectories from the given states and unpads the output.
* ``ActorCriticRecurrent(ActorCritic)``: the MLPs take ``rnn_hidden_size`` inputs; ``memory_a`` over the observations,
  ``memory_c`` over the critic observations, constructed after the MLPs.
* ``split_and_pad_trajectories`` / ``unpad_trajectories`` and ``recurrent_minibatch``: RolloutStorage's recurrent generator --
  minibatch i = envs [i N / nmb, (i + 1) N / nmb) over all T steps, no permutation; each trajectory (split at dones) starts from
  the state saved before its first step.
* ``minibatch_loss``: PPO.update's loss on such a minibatch (the formulas of oracle/ppo_torch.py, means over the T x mb rows).
"""
import torch
import torch.nn as nn

from oracle.ppo_torch import ActorCritic


def split_and_pad_trajectories(tensor, dones):
    """[T, N, ...] -> padded trajectories [T, num_traj, ...] (env-major, split after every done) and their masks [T, num_traj]."""
    dones = dones.clone()
    dones[-1] = 1
    flat_dones = dones.transpose(1, 0).reshape(-1, 1)
    done_indices = torch.cat((flat_dones.new_tensor([-1], dtype=torch.int64), flat_dones.nonzero()[:, 0]))
    trajectory_lengths = done_indices[1:] - done_indices[:-1]
    trajectories = torch.split(tensor.transpose(1, 0).flatten(0, 1), trajectory_lengths.tolist())
    trajectories = trajectories + (torch.zeros(tensor.shape[0], *tensor.shape[2:], device=tensor.device),)   # one full-length entry
    padded = torch.nn.utils.rnn.pad_sequence(trajectories)[:, :-1]
    masks = trajectory_lengths > torch.arange(0, tensor.shape[0], device=tensor.device).unsqueeze(1)
    return padded, masks


def unpad_trajectories(trajectories, masks):
    return trajectories.transpose(1, 0)[masks.transpose(1, 0)].view(-1, trajectories.shape[0], trajectories.shape[-1]).transpose(1, 0)


class Memory(nn.Module):
    def __init__(self, input_size, num_layers=1, hidden_size=256):
        super().__init__()
        self.rnn = nn.LSTM(input_size=input_size, hidden_size=hidden_size, num_layers=num_layers)
        self.hidden_states = None

    def forward(self, input, masks=None, hidden_states=None):
        if masks is not None:
            out, _ = self.rnn(input, hidden_states)
            return unpad_trajectories(out, masks)
        out, self.hidden_states = self.rnn(input.unsqueeze(0), self.hidden_states)
        return out

    def reset(self, dones=None):
        for h in self.hidden_states:
            h[..., dones, :] = 0.0


class ActorCriticRecurrent(ActorCritic):
    is_recurrent = True

    def __init__(self, num_actor_obs, num_critic_obs, num_actions, actor_hidden_dims, critic_hidden_dims, activation="elu",
                 rnn_hidden_size=256, rnn_num_layers=1, init_noise_std=1.0):
        super().__init__(rnn_hidden_size, rnn_hidden_size, num_actions, actor_hidden_dims, critic_hidden_dims, activation,
                         init_noise_std)
        self.memory_a = Memory(num_actor_obs, rnn_num_layers, rnn_hidden_size)
        self.memory_c = Memory(num_critic_obs, rnn_num_layers, rnn_hidden_size)

    def reset(self, dones=None):
        self.memory_a.reset(dones)
        self.memory_c.reset(dones)

    def act(self, obs, masks=None, hidden_states=None):
        return super().act(self.memory_a(obs, masks, hidden_states).squeeze(0))

    def act_inference(self, obs):
        return super().act_inference(self.memory_a(obs).squeeze(0))

    def evaluate(self, critic_obs, masks=None, hidden_states=None):
        return super().evaluate(self.memory_c(critic_obs, masks, hidden_states).squeeze(0))

    def get_hidden_states(self):
        return self.memory_a.hidden_states, self.memory_c.hidden_states


def recurrent_minibatch(st, mb, nmb):
    """Minibatch ``mb`` of the recurrent generator over storage ``st`` (dict of time-major tensors: obs, critic_obs, dones,
    saved_h_a, saved_c_a, saved_h_c, saved_c_c (T, N, H), actions, values, advantages, returns, log_prob, mu; sigma (A))."""
    T, N = st["dones"].shape
    dones = st["dones"].bool()
    pad_obs, masks = split_and_pad_trajectories(st["obs"], dones)
    pad_cobs, _ = split_and_pad_trajectories(st["critic_obs"], dones)
    mbs = N // nmb
    start, stop = mb * mbs, (mb + 1) * mbs
    last_was_done = torch.zeros_like(dones)
    last_was_done[1:] = dones[:-1]
    last_was_done[0] = True
    last_was_done = last_was_done.permute(1, 0)                      # env-major, the order of the split trajectories
    first_traj = int(torch.sum(last_was_done[:start]))
    last_traj = first_traj + int(torch.sum(last_was_done[start:stop]))
    hid = {}
    for k in ("h_a", "c_a", "h_c", "c_c"):
        s = st["saved_" + k].unsqueeze(1)                             # (T, layers = 1, N, H)
        hid[k] = s.permute(2, 0, 1, 3)[last_was_done][first_traj:last_traj].transpose(1, 0).contiguous()
    sl = slice(start, stop)
    return {"obs": pad_obs[:, first_traj:last_traj], "critic_obs": pad_cobs[:, first_traj:last_traj],
            "masks": masks[:, first_traj:last_traj], "hid_a": (hid["h_a"], hid["c_a"]), "hid_c": (hid["h_c"], hid["c_c"]),
            "actions": st["actions"][:, sl], "values": st["values"][:, sl].unsqueeze(-1),
            "advantages": st["advantages"][:, sl].unsqueeze(-1), "returns": st["returns"][:, sl].unsqueeze(-1),
            "log_prob": st["log_prob"][:, sl].unsqueeze(-1), "mu": st["mu"][:, sl], "sigma": st["sigma"].expand_as(st["mu"][:, sl])}


def minibatch_loss(ac, b, clip_param=0.2, value_loss_coef=1.0, entropy_coef=0.01, use_clipped_value_loss=True):
    ac.act(b["obs"], masks=b["masks"], hidden_states=b["hid_a"])
    logp = ac.get_actions_log_prob(b["actions"])
    value = ac.evaluate(b["critic_obs"], masks=b["masks"], hidden_states=b["hid_c"])
    mu, sigma, entropy = ac.action_mean, ac.action_std, ac.entropy
    with torch.no_grad():
        kl = torch.sum(torch.log(sigma / b["sigma"] + 1.e-5)
                       + (torch.square(b["sigma"]) + torch.square(b["mu"] - mu)) / (2.0 * torch.square(sigma)) - 0.5, axis=-1)
        kl_mean = torch.mean(kl)
    ratio = torch.exp(logp - torch.squeeze(b["log_prob"], -1))      # squeeze(-1): a bare squeeze also drops an env axis of one
    adv = torch.squeeze(b["advantages"], -1)
    surrogate_loss = torch.max(-adv * ratio, -adv * torch.clamp(ratio, 1.0 - clip_param, 1.0 + clip_param)).mean()
    if use_clipped_value_loss:
        value_clipped = b["values"] + (value - b["values"]).clamp(-clip_param, clip_param)
        value_loss = torch.max((value - b["returns"]).pow(2), (value_clipped - b["returns"]).pow(2)).mean()
    else:
        value_loss = (b["returns"] - value).pow(2).mean()
    loss = surrogate_loss + value_loss_coef * value_loss - entropy_coef * entropy.mean()
    return loss, kl_mean, value_loss, surrogate_loss
