"""F8: the reference's task wrappers (classification/class_task.py, regression/reg_task.py) on the device path -- the same
`(label, parameters)` constructors, attributes (`net`, `optimiser`, `scheduler`, `loss_info`, `epoch_loss`, `acc`,
`best_acc` / `best_loss`) and methods (`train_step`, `predict`, `evaluate`, `log_progress`), thin over the graphed training
steps: `train_step(train_data)` builds the step on first use and runs an epoch.EpochRunner when `train_data` is a
DeviceLoader, the reference's loop through `step.step` over any other iterable of (x, y).  The optimisers are FusedAdam /
FusedSGD (capturable) with the reference's StepLR on top; `log_progress` writes nothing unless a `writer` was given.  With
`histograms=True` the Bayesian tasks also write the reference's twelve weight histograms and its loss breakdown (F11)."""
from __future__ import annotations

import os

import numpy as np
import torch

from .epoch import DeviceLoader, EpochRunner, EvalLoader, evaluate as _evaluate, score as _score
from .optim import FusedAdam, FusedSGD


def _device():
    import config
    return config.DEVICE


class _Task:
    _keys = ()
    bayesian = True

    def __init__(self, label, parameters, writer=None, histograms=False):
        self.writer = writer
        self._histograms, self._stats = bool(histograms), None
        self.label = label
        for attr, key in self._keys:
            setattr(self, attr, parameters[key])
        self.save_model_path = f'{parameters["save_dir"]}/{label}_model.pt'
        self._steps, self._runners = {}, {}
        self.init_net(parameters)

    # ---- the graphed step of a minibatch shape, and the runner of a loader
    def _make_step(self, x, y):
        raise NotImplementedError

    def _step_for(self, x, y):
        key = (tuple(x.shape), tuple(y.shape))
        if key not in self._steps:
            self._steps[key] = self._make_step(x, y)
        return self._steps[key]

    def _runner(self, loader: DeviceLoader) -> EpochRunner:
        if id(loader) not in self._runners:
            self._runners[id(loader)] = EpochRunner(self._step_for(*loader.example()), loader)
        return self._runners[id(loader)]

    def _loss_info(self, row):
        """A history row shaped as the reference's loss_info."""
        if not self.bayesian:
            return row[0]
        if len(row) == 4:
            return row[0:1], row[1], row[2], row[3:4]
        return row[0:1], row[1], row[2:3]

    def train_step(self, train_data):
        self.net.train()
        if isinstance(train_data, DeviceLoader):
            self.loss_history = self._runner(train_data).run_epoch()
            self.loss_info = self._loss_info(self.loss_history[-1])
        else:
            dev = _device()
            for idx, (x, y) in enumerate(train_data):
                x, y = x.to(dev), y.to(dev)
                step = self._step_for(x, y)
                if self.bayesian:
                    beta = 2 ** (self.num_batches - (idx + 1)) / (2 ** self.num_batches - 1)
                    self.loss_info = step.step(x, y, beta)
                else:
                    self.loss_info = step.step(x, y)
        self._after_epoch()

    def _after_epoch(self):
        pass

    def log_progress(self, step):
        if self.writer is None:
            return
        loss = self.loss_info[0] if self.bayesian else self.loss_info
        self.writer.add_scalar("loss", float(loss), step)
        if hasattr(self, "acc"):
            self.writer.add_scalar("accuracy", self.acc, step)
        if self._histograms and self.bayesian:
            self._log_posterior(step)

    def _log_posterior(self, step):
        """The reference's Bayesian logging (utils/logger_utils.py:13-39): write_weight_histograms from one device pass and
        one copy (diagnostics.PosteriorStats), write_loss_scalars from loss_info."""
        from . import diagnostics
        if self._stats is None:
            self._stats = diagnostics.PosteriorStats(self.net)
        for tag, fields in self._stats.update().read().items():
            self.writer.add_histogram_raw(tag, **fields, global_step=step)
        loss = [float(v) for v in self.loss_info]
        self.writer.add_scalar("logs/loss", loss[0], step)
        if len(loss) == 4:
            self.writer.add_scalar("logs/complexity_cost", loss[2] - loss[1], step)
            self.writer.add_scalar("logs/log_prior", loss[1], step)
            self.writer.add_scalar("logs/log_variational_posterior", loss[2], step)
            self.writer.add_scalar("logs/negative_log_likelihood", loss[3], step)
        else:
            self.writer.add_scalar("logs/complexity_cost", loss[1], step)
            self.writer.add_scalar("logs/negative_log_likelihood", loss[2], step)


def _makedirs(parameters):
    if not os.path.exists(parameters["save_dir"]):
        os.makedirs(parameters["save_dir"])


def _bnn_params(t, parameters, classes, hidden, mode):
    return {'input_shape': t.x_shape, 'classes': classes, 'batch_size': t.batch_size, 'hidden_units': hidden, 'mode': mode,
            'mu_init': parameters['mu_init'], 'rho_init': parameters['rho_init'], 'prior_init': parameters['prior_init'],
            'mixture_prior': parameters['mixture_prior'], 'local_reparam': t.local_reparam}


# ------------------------------------------------------------------------------------------------------- classification
class _ClassTask(_Task):
    def init_net(self, parameters):
        raise NotImplementedError

    def evaluate(self, test_loader):
        self.net.eval()
        if isinstance(test_loader, DeviceLoader):
            correct, total = _evaluate(self.net, test_loader, self._eval_samples()), len(test_loader) * self.batch_size
        else:
            dev = _device()
            correct = torch.zeros((), dtype=torch.int64, device=dev)
            total = 0
            with torch.no_grad():
                for X, y in test_loader:
                    X, y = X.to(dev), y.to(dev)
                    preds, _ = self.predict(X)
                    total += self.batch_size
                    correct += (preds == y).sum()
            correct = int(correct.item())
        self.acc = correct / total

    def score(self, test_loader, bins=10):
        """The held-out scores of the test set (epoch.score: log predictive density, expected NLL, Brier, accuracy, ECE /
        MCE and the reliability bins) at the task's test_samples -- the read() result, one copy."""
        self.net.eval()
        if not isinstance(test_loader, (DeviceLoader, EvalLoader)):
            raise TypeError("score: a bnn_hip.epoch.DeviceLoader or EvalLoader over the test set is needed")
        return _score(self.net, test_loader, self._eval_samples(), bins=bins).read()

    def _eval_samples(self):
        return 0


class BNN_Classification(_ClassTask):
    _keys = (("lr", "lr"), ("hidden_units", "hidden_units"), ("mode", "mode"), ("batch_size", "batch_size"),
             ("num_batches", "num_batches"), ("n_samples", "train_samples"), ("test_samples", "test_samples"),
             ("x_shape", "x_shape"), ("classes", "classes"), ("mu_init", "mu_init"), ("rho_init", "rho_init"),
             ("prior_init", "prior_init"), ("mixture_prior", "mixture_prior"), ("local_reparam", "local_reparam"))

    def init_net(self, parameters):
        import networks
        _makedirs(parameters)
        self.best_acc = 0.
        self.net = networks.BayesianNetwork(_bnn_params(self, parameters, self.classes, self.hidden_units, self.mode)).to(_device())
        self.optimiser = FusedAdam(self.net.parameters(), lr=self.lr, capturable=True)
        self.scheduler = torch.optim.lr_scheduler.StepLR(self.optimiser, step_size=100, gamma=0.5)

    def _make_step(self, x, y):
        from .train import GraphedTrainStep
        return GraphedTrainStep(self.net, self.optimiser, x, y, self.n_samples)

    def predict(self, X):
        return self.net.predict_mc(X, self.test_samples)

    def _eval_samples(self):
        return self.test_samples


class MLP_Classification(_ClassTask):
    bayesian = False
    _keys = (("lr", "lr"), ("hidden_units", "hidden_units"), ("mode", "mode"), ("batch_size", "batch_size"),
             ("num_batches", "num_batches"), ("x_shape", "x_shape"), ("classes", "classes"), ("dropout", "dropout"))

    def init_net(self, parameters):
        import networks
        _makedirs(parameters)
        self.best_acc = 0.
        model_params = {'input_shape': self.x_shape, 'classes': self.classes, 'batch_size': self.batch_size,
                        'hidden_units': self.hidden_units, 'mode': self.mode, 'dropout': self.dropout}
        self.net = (networks.MLP_Dropout if self.dropout else networks.MLP)(model_params).to(_device())
        self.optimiser = FusedSGD(self.net.parameters(), lr=self.lr, capturable=True)
        self.scheduler = torch.optim.lr_scheduler.StepLR(self.optimiser, step_size=100, gamma=0.5)

    def _make_step(self, x, y):
        return self.net.graphed_train_step(self.optimiser, x, y)

    def predict(self, X):
        probs = torch.nn.Softmax(dim=1)(self.net(X))
        return torch.argmax(probs, dim=1), probs


class MCDropout_Classification(MLP_Classification):
    _keys = MLP_Classification._keys + (("test_samples", "test_samples"),)

    def init_net(self, parameters):
        self.dropout = True                      # the reference builds MLP_Dropout whatever the key says
        super().init_net(parameters)

    def predict(self, X):
        return self.net.predict_mc(X, self.test_samples)

    def _eval_samples(self):
        return self.test_samples


# ----------------------------------------------------------------------------------------------------------- regression
class _RegTask(_Task):
    def _after_epoch(self):
        self.epoch_loss = float(self.loss_info[0] if self.bayesian else self.loss_info)      # one read per epoch

    def _score(self, x_test, y_test, bins):
        """net.score on the whole test set as one minibatch, sigma = the NLL's noise_tolerance: the read() result."""
        self.net.eval()
        dev = _device()
        x = torch.as_tensor(x_test, dtype=torch.float32).to(dev)
        y = torch.as_tensor(y_test, dtype=torch.float32).to(dev).reshape(x.shape[0], -1)
        with torch.no_grad():
            return self.net.score(x, y, self.test_samples, sigma=self.noise_tol, bins=bins).read()


class BNN_Regression(_RegTask):
    _keys = (("batch_size", "batch_size"), ("num_batches", "num_batches"), ("n_samples", "train_samples"),
             ("test_samples", "test_samples"), ("x_shape", "x_shape"), ("y_shape", "y_shape"),
             ("noise_tol", "noise_tolerance"), ("lr", "lr"), ("local_reparam", "local_reparam"))

    def init_net(self, parameters):
        import networks
        _makedirs(parameters)
        self.best_loss = np.inf
        self.net = networks.BayesianNetwork(_bnn_params(self, parameters, self.y_shape, parameters['hidden_units'],
                                                        parameters['mode'])).to(_device())
        self.optimiser = FusedAdam(self.net.parameters(), lr=self.lr, capturable=True)
        self.scheduler = torch.optim.lr_scheduler.StepLR(self.optimiser, step_size=500, gamma=0.5)

    def _make_step(self, x, y):
        from .train import GraphedTrainStep
        return GraphedTrainStep(self.net, self.optimiser, x, y, self.n_samples, sigma=self.noise_tol)

    def predict(self, X):
        """[test_samples, n, out]: the stochastic forward passes evaluate() collects."""
        return self.net.forward_mc(X, self.test_samples)

    def evaluate(self, x_test):
        self.net.eval()
        with torch.no_grad():
            y = self.predict(x_test.to(_device()))
            return y.reshape(self.test_samples, -1).double().cpu().numpy()

    def score(self, x_test, y_test, bins=10):
        """The held-out scores of (x_test, y_test) under the N(f_s, noise_tolerance^2) mixture of test_samples passes: log
        predictive density and expected NLL per element, RMSE / MAE of the predictive mean, the PIT histogram with
        coverage(level)."""
        return self._score(x_test, y_test, bins)


class MLP_Regression(_RegTask):
    bayesian = False
    _keys = (("lr", "lr"), ("hidden_units", "hidden_units"), ("mode", "mode"), ("batch_size", "batch_size"),
             ("num_batches", "num_batches"), ("x_shape", "x_shape"), ("y_shape", "y_shape"))
    _sched_step = 5000
    _dropout = False

    def init_net(self, parameters):
        import networks
        _makedirs(parameters)
        self.best_loss = np.inf
        model_params = {'input_shape': self.x_shape, 'classes': self.y_shape, 'batch_size': self.batch_size,
                        'hidden_units': self.hidden_units, 'mode': self.mode}
        self.net = (networks.MLP_Dropout if self._dropout else networks.MLP)(model_params).to(_device())
        self.optimiser = FusedAdam(self.net.parameters(), lr=self.lr, capturable=True)
        self.scheduler = torch.optim.lr_scheduler.StepLR(self.optimiser, step_size=self._sched_step, gamma=0.5)

    def _make_step(self, x, y):
        return self.net.graphed_train_step(self.optimiser, x, y)

    def predict(self, X):
        return self.net(X)

    def evaluate(self, x_test):
        self.net.eval()
        with torch.no_grad():
            return self.predict(x_test.to(_device())).detach().cpu().numpy()


class MCDropout_Regression(MLP_Regression):
    _keys = MLP_Regression._keys + (("test_samples", "test_samples"),)
    _sched_step = 500
    _dropout = True

    def init_net(self, parameters):
        super().init_net(parameters)
        self.noise_tol = float(parameters.get("noise_tolerance", 1.0))     # score()'s sigma; the reference's wrapper has none

    def predict(self, X):
        """[test_samples, n, out]: the MC-dropout passes evaluate() collects."""
        return self.net.mc_forward(X, self.test_samples)

    def evaluate(self, x_test):
        self.net.eval()
        with torch.no_grad():
            y = self.predict(x_test.to(_device()))
            return y.reshape(self.test_samples, -1).double().cpu().numpy()

    def score(self, x_test, y_test, bins=10):
        """As BNN_Regression.score, over test_samples MC-dropout passes.  The reference gives this wrapper no
        noise_tolerance: `noise_tol` (1.0 unless the parameters carry "noise_tolerance") is the mixture's sigma."""
        return self._score(x_test, y_test, bins)
