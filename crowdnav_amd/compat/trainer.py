"""Replay memory and SGD trainer on the reference's interfaces (crowd_nav/utils/memory.py:4-28,
trainer.py:8-71).  They stay plain PyTorch (ROCm) exactly as BASELINE configs[4] asks: the rollouts come from the
HIP engine, the optimizer from torch.  When the reference is importable its own classes can be used instead.
Opt-in (CROWDNAV_AMD_SGD_KERNEL=1, default 0): a sarl.ValueNetwork or an lstm_rl.ValueNetwork1 on a GPU with a DeviceReplayMemory
on the same device takes its SGD steps through cn_train_step instead — two HIP launches per batch on the same parameter tensors
and on momentum buffers installed in the torch optimizer's state, so the two paths can follow each other within one run."""
import logging
import os

import torch
import torch.nn as nn
import torch.optim as optim
from torch.utils.data import DataLoader, Dataset


class ReplayMemory(Dataset):
    """Ring buffer of (state [H, D] float32, value [1] float32) pairs."""

    def __init__(self, capacity):
        self.capacity = capacity
        self.memory = []
        self.position = 0

    def push(self, item):
        if self.position < len(self.memory):
            self.memory[self.position] = item
        else:
            self.memory.append(item)
        self.position = (self.position + 1) % self.capacity

    def is_full(self):
        return len(self.memory) == self.capacity

    def __getitem__(self, item):
        return self.memory[item]

    def __len__(self):
        return len(self.memory)

    def clear(self):
        self.memory = []


class DeviceReplayMemory(Dataset):
    """The same ring (memory.py:4-28: push order, overwrite from position 0 once full) held as two device tensors —
    states [capacity, H, D] and values [capacity, 1] float32 — so that a batched rollout pushes all its (state, value)
    pairs with one index_copy (push_batch) and the trainer draws batches with one gather (no DataLoader, no per-item
    collate).  Still a Dataset of (state, value) pairs for code that iterates it the reference's way."""

    def __init__(self, capacity, device='cuda:0'):
        self.capacity = int(capacity)
        self.device = torch.device(device)
        self.states = None
        self.values = torch.zeros(self.capacity, 1, dtype=torch.float32, device=self.device)
        self.size = 0
        self.position = 0

    def push_batch(self, states, values):
        """states [n, ...] and values [n] (or [n, 1]) in push order; equivalent to n push() calls."""
        n = int(states.shape[0])
        if n == 0:
            return
        states = states.to(device=self.device, dtype=torch.float32)
        values = values.to(device=self.device, dtype=torch.float32).reshape(n, 1)
        if self.states is None:
            self.states = torch.zeros((self.capacity,) + tuple(states.shape[1:]), dtype=torch.float32,
                                      device=self.device)
        if n > self.capacity:  # only the last `capacity` pushes survive; the ring position still advances by n
            self.position = (self.position + n - self.capacity) % self.capacity
            states, values, n_eff = states[-self.capacity:], values[-self.capacity:], self.capacity
        else:
            n_eff = n
        head = min(n_eff, self.capacity - self.position)  # rows up to the end of the ring: two plain copies, not five kernels
        self.states[self.position:self.position + head].copy_(states[:head])
        self.values[self.position:self.position + head].copy_(values[:head])
        if head < n_eff:  # the rest wraps round
            self.states[:n_eff - head].copy_(states[head:])
            self.values[:n_eff - head].copy_(values[head:])
        self.position = (self.position + n_eff) % self.capacity
        self.size = min(self.capacity, self.size + n)

    def push(self, item):
        state, value = item
        self.push_batch(state.unsqueeze(0), value.reshape(1))

    def is_full(self):
        return self.size == self.capacity

    def __getitem__(self, index):
        if not -self.size <= index < self.size:
            raise IndexError(index)
        return self.states[index], self.values[index]

    def __len__(self):
        return self.size

    def clear(self):
        self.size = 0
        self.position = 0

    def batches(self, batch_size, limit=None):
        """One shuffled pass (DataLoader(shuffle=True) semantics: a random permutation cut into batches, the last one
        partial); limit = number of batches to yield."""
        perm = torch.randperm(self.size, device=self.device)
        stops = range(0, self.size, batch_size)
        for n, start in enumerate(stops):
            if limit is not None and n >= limit:
                return
            idx = perm[start:start + batch_size]
            yield self.states.index_select(0, idx), self.values.index_select(0, idx)


class Trainer(object):
    """SGD(momentum 0.9) + MSE on the value network; optimize_epoch for imitation learning, optimize_batch for RL."""

    def __init__(self, model, memory, device, batch_size):
        self.model = model
        self.device = device
        self.criterion = nn.MSELoss().to(device)
        self.memory = memory
        self.data_loader = None
        self.batch_size = batch_size
        self.optimizer = None
        self._graph = None          # hipGraph of one full-batch SGD step (device memory on a GPU only)
        self._graph_failed = os.environ.get('CROWDNAV_AMD_SGD_GRAPH', '1') == '0'
        self._kernel_on = os.environ.get('CROWDNAV_AMD_SGD_KERNEL', '0') == '1'  # device SGD step (cn_train_step), opt-in
        self._kernel_off = False    # ... refused for this model / memory: today's path for the rest of the run
        self._kstep = None          # crowdnav_amd.train.SarlTrainStep / LstmTrainStep
        self._kshape = None         # (H, D) of the memory the handle was made for
        self._kopt = None           # the optimizer whose momentum buffers the handle is bound to

    def set_learning_rate(self, learning_rate):
        logging.info('Current learning rate: %f', learning_rate)
        self.optimizer = optim.SGD(self.model.parameters(), lr=learning_rate, momentum=0.9)
        self._graph = None  # the captured step belongs to the previous optimizer

    def _capture(self, inputs, values):
        """Capture forward + backward + SGD update of one full batch into a graph (the step is ~60 tiny kernels:
        launch-bound).  Warm-up iterations run on a side stream as torch requires; parameters and momentum buffers are
        put back afterwards, so capturing does not train."""
        params = [p for g in self.optimizer.param_groups for p in g['params']]
        saved = [p.detach().clone() for p in params]
        had = [('momentum_buffer' in self.optimizer.state.get(p, {})
                and self.optimizer.state[p]['momentum_buffer'] is not None) for p in params]
        saved_buf = [self.optimizer.state[p]['momentum_buffer'].clone() if h else None for p, h in zip(params, had)]
        self._sx, self._sy = inputs.clone(), values.clone()
        try:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(3):
                    self.optimizer.zero_grad(set_to_none=True)
                    self.criterion(self.model(self._sx), self._sy).backward()
                    self.optimizer.step()
            torch.cuda.current_stream().wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            self.optimizer.zero_grad(set_to_none=True)
            with torch.cuda.graph(graph):
                self._sloss = self.criterion(self.model(self._sx), self._sy)
                self._sloss.backward()
                self.optimizer.step()
        finally:
            with torch.no_grad():
                for p, keep, h, buf in zip(params, saved, had, saved_buf):
                    p.copy_(keep)
                    mb = self.optimizer.state.get(p, {}).get('momentum_buffer')
                    if mb is not None:
                        mb.copy_(buf) if h else mb.zero_()  # a zero buffer == no buffer for the next update
        self._graph = graph

    def _fit_graph(self, inputs, values):
        if self._graph is None:
            self._capture(inputs, values)
        self._sx.copy_(inputs)
        self._sy.copy_(values)
        self._graph.replay()
        self._bump()
        return self._sloss.detach().clone()

    def _loader(self):
        if self.optimizer is None:
            raise ValueError('Learning rate is not set!')
        if self.data_loader is None:
            self.data_loader = DataLoader(self.memory, self.batch_size, shuffle=True)
        return self.data_loader

    def _bump(self):
        """Tell device-side consumers of the parameters that they changed: a replayed graph updates them without touching
        the tensors' version counters, so CrowdSim.sarl_action keys its re-upload on this counter as well."""
        self.model._cn_weights_epoch = getattr(self.model, '_cn_weights_epoch', 0) + 1

    def _fit(self, inputs, values):
        self.optimizer.zero_grad()
        loss = self.criterion(self.model(inputs.to(self.device)), values.to(self.device))
        loss.backward()
        self.optimizer.step()
        self._bump()
        return loss.data.item()

    def _fit_device(self, inputs, values):
        """_fit without the per-batch host sync: the loss stays a device scalar.  Full batches on a GPU replay the
        captured step."""
        if inputs.is_cuda and inputs.shape[0] == self.batch_size and not self._graph_failed:
            try:
                return self._fit_graph(inputs, values)
            except Exception as exc:  # capture unsupported in this build: the eager step below is always valid
                logging.warning('SGD step graph capture failed (%s); running eagerly', exc)
                self._graph, self._graph_failed = None, True
        self.optimizer.zero_grad()
        loss = self.criterion(self.model(inputs), values)
        loss.backward()
        self.optimizer.step()
        self._bump()
        return loss.detach()

    def _device_memory(self):
        return (isinstance(self.memory, DeviceReplayMemory) and self.memory.device == torch.device(self.device)
                and len(self.memory) > 0)

    def _kernel_refused(self, why):
        logging.warning('CROWDNAV_AMD_SGD_KERNEL=1: %s; the SGD steps stay on PyTorch', why)
        self._kernel_off = True
        return None

    def _kernel(self):
        """The device SGD step bound to this model, optimizer and memory, or None where today's path applies: switch off,
        a CPU model, a list-backed memory (silently: nothing was asked of a GPU), or a model / size the library has no
        step for (one log line, then today's path for the rest of the run)."""
        if not self._kernel_on or self._kernel_off or not self._device_memory():
            return None
        states = self.memory.states
        params = [p for g in self.optimizer.param_groups for p in g['params']]
        if states is None or not states.is_cuda or not params or any(p.device != states.device for p in params):
            return None
        from .lstm_rl import ValueNetwork1
        from .sarl import ValueNetwork
        if not isinstance(self.model, (ValueNetwork, ValueNetwork1)):
            return self._kernel_refused('%s.%s has no device SGD step' % (type(self.model).__module__.rsplit('.', 1)[-1],
                                                                                   type(self.model).__name__))
        group = self.optimizer.param_groups[0]
        if (len(self.optimizer.param_groups) != 1 or group.get('dampening', 0) or group.get('weight_decay', 0)
                or group.get('nesterov', False) or group.get('maximize', False)):
            return self._kernel_refused('the optimizer is not plain SGD with momentum')
        shape = tuple(states.shape[1:])
        if self._kstep is None or self._kshape != shape:
            from .. import train as cn_train
            from .._lib import CN_ERR_UNSUPPORTED, CrowdNavAmdError
            try:
                if states.dim() != 3:
                    raise CrowdNavAmdError(CN_ERR_UNSUPPORTED, 'memory states of shape %s' % (tuple(states.shape),))
                make = cn_train.LstmTrainStep if isinstance(self.model, ValueNetwork1) else cn_train.SarlTrainStep
                self._kstep = make(cn_train.module_net_config(self.model), shape[0], self.batch_size, states.device.index or 0)
            except CrowdNavAmdError as exc:
                if exc.status != CN_ERR_UNSUPPORTED:
                    raise
                return self._kernel_refused(str(exc))
            self._kshape, self._kopt = shape, None
        if self._kopt is not self.optimizer:  # a new optimizer starts from zero buffers, as torch's does
            bufs = []
            for p in params:
                st = self.optimizer.state[p]
                if st.get('momentum_buffer') is None:
                    st['momentum_buffer'] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                bufs.append(st['momentum_buffer'])
            self._kstep.bind([p.data for p in params], bufs)
            self._kopt = self.optimizer
        return self._kstep

    def _fit_kernel(self, kstep, index, total):
        """One device SGD step on the ring rows `index` names; the batch's MSE is added to the float64 device scalar total."""
        group = self.optimizer.param_groups[0]
        kstep.step(self.memory.states, self.memory.values, index, int(index.numel()), group['lr'], group['momentum'], total)
        self._bump()

    def _draw_batches(self, count):
        """Index sets of `count` batches, each the head of a fresh uniform permutation of the memory (trainer.py:57): the
        batch_size largest of one i.i.d. uniform float64 key per row — a uniformly random ordered subset without duplicates,
        since every ordering of distinct keys is equally likely.  Drawn a chunk of batches at a time (two kernels per
        chunk instead of a sort per batch); the random stream differs from the torch path's randperm."""
        size, k = len(self.memory), min(self.batch_size, len(self.memory))
        chunk = max(1, min(count, (1 << 22) // size))
        done = 0
        while done < count:
            c = min(chunk, count - done)
            keys = torch.rand(c, size, dtype=torch.float64, device=self.memory.device)
            for row in keys.topk(k, dim=1).indices:
                yield row
            done += c

    def optimize_epoch(self, num_epochs):
        if self.optimizer is None:
            raise ValueError('Learning rate is not set!')
        kstep = self._kernel()
        if kstep is not None:
            average_epoch_loss = 0
            for epoch in range(num_epochs):
                total = torch.zeros((), dtype=torch.float64, device=self.memory.device)
                perm = torch.randperm(self.memory.size, device=self.memory.device)
                for start in range(0, self.memory.size, self.batch_size):
                    self._fit_kernel(kstep, perm[start:start + self.batch_size], total)
                average_epoch_loss = total.item() / len(self.memory)
                logging.debug('Average loss in epoch %d: %.2E', epoch, average_epoch_loss)
            return average_epoch_loss
        if self._device_memory():
            average_epoch_loss = 0
            for epoch in range(num_epochs):
                total = torch.zeros((), device=self.memory.device)
                for inputs, values in self.memory.batches(self.batch_size):
                    total += self._fit_device(inputs, values)
                average_epoch_loss = total.item() / len(self.memory)
                logging.debug('Average loss in epoch %d: %.2E', epoch, average_epoch_loss)
            return average_epoch_loss
        loader = self._loader()
        average_epoch_loss = 0
        for epoch in range(num_epochs):
            epoch_loss = sum(self._fit(inputs, values) for inputs, values in loader)
            average_epoch_loss = epoch_loss / len(self.memory)
            logging.debug('Average loss in epoch %d: %.2E', epoch, average_epoch_loss)
        return average_epoch_loss

    def optimize_batch(self, num_batches):
        if self.optimizer is None:
            raise ValueError('Learning rate is not set!')
        kstep = self._kernel()
        if kstep is not None:
            total = torch.zeros((), dtype=torch.float64, device=self.memory.device)
            for index in self._draw_batches(num_batches):
                self._fit_kernel(kstep, index, total)
            average_loss = total.item() / num_batches
            logging.debug('Average loss : %.2E', average_loss)
            return average_loss
        if self._device_memory():
            total = torch.zeros((), device=self.memory.device)
            for _ in range(num_batches):  # a fresh permutation per batch, as trainer.py:57 does
                inputs, values = next(self.memory.batches(self.batch_size, limit=1))
                total += self._fit_device(inputs, values)
            average_loss = total.item() / num_batches
            logging.debug('Average loss : %.2E', average_loss)
            return average_loss
        loader = self._loader()
        losses = 0
        for _ in range(num_batches):
            inputs, values = next(iter(loader))  # a fresh shuffled iterator per batch, as trainer.py:57 does
            losses += self._fit(inputs, values)
        average_loss = losses / num_batches
        logging.debug('Average loss : %.2E', average_loss)
        return average_loss
