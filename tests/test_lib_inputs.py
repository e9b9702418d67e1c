"""The binding's one input path (_lib._obs) as every entry point uses it:
inconsistent host batches and tensors that are not on the GPU raise ValueError
before any library call that could reach a device.  CPU only."""
import numpy as np
import pytest
import torch

from optimalinterpolation_amd import _lib

N, M = 6, 2
P = 6 + 4 * M + M * (M + 1) // 2
X0_6 = np.zeros(6)
HYP = np.ones((2, 5))
SEL, SOFFS = np.array([0, 1, 0, 1]), [0, 2, 4]
XS = np.zeros((2, 3))

# name -> call(xyt, y, offs, **kw) on a batch of two cells
ONE_SHOT = {
    'gpr_batch': lambda x, y, o, **k: _lib.gpr_batch(x, y, o, XS, 0.0, x0=X0_6, **k),
    'nlml_grad_batch': lambda x, y, o, **k: _lib.nlml_grad_batch(x, y, np.zeros(len(y)), o,
                                                                 np.zeros((2, 6)), **k),
    'gpr_predict_multi': lambda x, y, o, **k: _lib.gpr_predict_multi(x, y, o, XS, [0, 1, 2], 0.0, HYP, **k),
    'nystrom_batch': lambda x, y, o, **k: _lib.nystrom_batch(x, y, o, SEL, SOFFS, HYP, xs=XS, **k),
    'nystrom_fit_batch': lambda x, y, o, **k: _lib.nystrom_fit_batch(x, y, o, SEL, SOFFS, np.zeros(5),
                                                                     XS, 0.0, **k),
    'svgp_batch': lambda x, y, o, **k: _lib.svgp_batch(x, y, o, np.zeros((2, M, 3)), np.ones((2, 6)), XS,
                                                       batch=4, iterations=1, **k),
    'svgp_elbo': lambda x, y, o, **k: _lib.svgp_elbo(np.zeros((2, P)), x, y, o, **k),
}
# the entries that take device tensors, as callables of (xyt, y, offs)
DEVICE = {
    'gpr_batch_device': lambda x, y, o: _lib.gpr_batch_device(x, y, o, XS, 0.0, x0=X0_6),
    'gpr_predict_multi_device': lambda x, y, o: _lib.gpr_predict_multi_device(x, y, o, XS, [0, 1, 2], 0.0, HYP),
    'nystrom_fit_batch': lambda x, y, o: ONE_SHOT['nystrom_fit_batch'](x, y, o, device_inputs=True),
    'svgp_batch': lambda x, y, o: ONE_SHOT['svgp_batch'](x, y, o, device_inputs=True),
    'svgp_elbo': lambda x, y, o: ONE_SHOT['svgp_elbo'](x, y, o, device_inputs=True),
}


@pytest.mark.parametrize('name', list(ONE_SHOT))
@pytest.mark.parametrize('rows, ny, offs', [
    (N, N, [1, 3, N]),          # offs[0] != 0
    (N, N, [0, 3, N - 1]),      # offs[-1] != len(y)
    (N - 1, N, [0, 3, N]),      # rows(xyt) != len(y)
], ids=['offs0', 'offs_end', 'rows'])
def test_inconsistent_host_batch_is_value_error(name, rows, ny, offs):
    with pytest.raises(ValueError):
        ONE_SHOT[name](np.zeros((rows, 3)), np.zeros(ny), offs)


@pytest.mark.parametrize('name', list(DEVICE))
def test_cpu_tensor_as_device_input_is_value_error(name):
    with pytest.raises(ValueError, match='cuda'):
        DEVICE[name](torch.zeros(N, 3, dtype=torch.float64), torch.zeros(N, dtype=torch.float64), [0, 3, N])


def test_svgp_predict_cpu_tensor_targets_is_value_error():
    with pytest.raises(ValueError, match='cuda'):
        _lib.svgp_predict(np.zeros((2, P)), torch.zeros(2, 3, dtype=torch.float64), [0, 1, 2],
                          device_inputs=True)


def test_gpr_batch_device_checks_x0_and_hyp_like_gpr_batch():
    x, y = torch.zeros(N, 3, dtype=torch.float64), torch.zeros(N, dtype=torch.float64)
    for call, xx, yy in ((_lib.gpr_batch, x.numpy(), y.numpy()), (_lib.gpr_batch_device, x, y)):
        with pytest.raises(ValueError, match='opt=True needs x0'):
            call(xx, yy, [0, 3, N], XS, 0.0, opt=True)
        with pytest.raises(ValueError, match='opt=False needs hyp'):
            call(xx, yy, [0, 3, N], XS, 0.0, opt=False)
        with pytest.raises(ValueError, match='opt=False needs hyp'):
            call(xx, yy, [0, 3, N], XS, 0.0, opt=False, hyp=np.ones((3, 5)))
