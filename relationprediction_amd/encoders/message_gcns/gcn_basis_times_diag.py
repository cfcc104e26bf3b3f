"""Basis layer with per-feature coefficients `BasisGcnTimesDiag` (reference:
code/encoders/message_gcns/gcn_basis_times_diag.py; selected by DiagonalCoefficients=Yes, model_builder.py:287-288,
ahead of Concatenation).

W_r = sum_b W_b . diag(sigmoid(C[r, b, :])): message = sum_b sigmoid(C[r,b,:]) * (x . W[:, b, :]) (:44-73).  Weights
and their creation order (:20-35): W_forward, W_backward `[d, B, d]` (in, basis, out), W_self `[d, d]`, all
N(0, glorot_variance([d, d])); C_forward, C_backward `[R, B, d]` ~ N(0, 1); b = 0.  Unlike BasisGcn and ConcatGcn
 the bias IS added (:86): it has a gradient and the optimizer moves it.
`get_weights()` order (:38-42): W_forward, W_backward, C_forward, C_backward, W_self, b.

The reference's parse_settings also does int(settings['GraphSplitSize']) (:12), which dies on the shipped
`GraphSplitSize=0.5`; nothing in the layer uses the value, so it is not read here and any value is accepted.
The one-hot first layer (UseInputTransform=No) and highway wrappers are not built for this layer (model_builder
refuses both).  Engine: csrc/basis_tdiag.hip (RGCN_KIND_BASIS_TDIAG).
"""
from ...common.shared_functions import glorot_variance, make_variable, make_bias
from ...model import Variable
from .message_gcn import MessageGcn


class BasisGcnTimesDiag(MessageGcn):
    KIND = "basis_tdiag"

    def parse_settings(self):
        self.dropout_keep_probability = float(self.settings['DropoutKeepProbability'])
        self.n_coefficients = int(self.settings['NumberOfBasisFunctions'])

    def create_variables(self):
        if self.onehot_input:
            raise NotImplementedError("DiagonalCoefficients=Yes with UseInputTransform=No: the one-hot first layer of "
                                      "BasisGcnTimesDiag is not built")
        d_in, d_out = self.shape[0], self.shape[1]
        type_matrix_shape = (self.relation_count, self.n_coefficients, d_out)
        vertex_matrix_shape = (d_in, self.n_coefficients, d_out)
        self_matrix_shape = (d_in, d_out)
        var = glorot_variance([vertex_matrix_shape[0], vertex_matrix_shape[2]])
        self.W_forward = Variable("W_forward", vertex_matrix_shape, make_variable(0, var, vertex_matrix_shape))
        self.W_backward = Variable("W_backward", vertex_matrix_shape, make_variable(0, var, vertex_matrix_shape))
        self.W_self = Variable("W_self", self_matrix_shape, make_variable(0, var, self_matrix_shape))
        self.C_forward = Variable("C_forward", type_matrix_shape, make_variable(0, 1, type_matrix_shape))
        self.C_backward = Variable("C_backward", type_matrix_shape, make_variable(0, 1, type_matrix_shape))
        self.b = Variable("b", (d_out,), make_bias(d_out))

    def engine_variables(self):
        return [(self.W_forward, "W_f"), (self.W_backward, "W_b"), (self.C_forward, "C_f"),
                (self.C_backward, "C_b"), (self.W_self, "W_self"), (self.b, "b")]

    def local_get_weights(self):
        return [self.W_forward, self.W_backward, self.C_forward, self.C_backward, self.W_self, self.b]

    def local_get_regularization(self):
        return 0.0      # the reference class defines none: the chain's base 0 (model.py:111-112)
