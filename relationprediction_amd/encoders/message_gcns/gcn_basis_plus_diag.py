"""Basis layer with a per-relation diagonal `BasisGcnWithDiag` (reference:
code/encoders/message_gcns/gcn_basis_plus_diag.py; selected by AddDiagonal=Yes, model_builder.py:285-286, the flag the
reference checks first).

The basis layer plus a DistMult-like term per message, `H[src] * D[r]`, with a trained vector per directed relation, and a
bias that IS added and trained (:102), unlike BasisGcn and ConcatGcn.  What the reference executes is built,
not what its names suggest: compute_messages unpacks the two basis products the other way round from how
compute_basis_functions returns them (:51 against :75-79), so the basis term of a message is formed from the
DESTINATION's own features under the OTHER direction's basis tensor.

Weights and their creation order (:27-39): W_forward, W_backward `[d, B, d]` (in, basis, out), W_self `[d, d]`, all
N(0, glorot_variance([d, d])); C_forward, C_backward `[R, B]`, D_types_forward, D_types_backward `[R, d]` ~ N(0, 1); b = 0.
`get_weights()` order (:42-47): W_forward, W_backward, C_forward, C_backward, D_types_backward, D_types_forward, W_self, b
-- the BACKWARD diagonal table first; both are `[R, d]`, so no shape check catches a mix-up.

The reference's parse_settings also does int(settings['GraphSplitSize']) (:12), which dies on the shipped
`GraphSplitSize=0.5`; nothing in the layer uses the value, so it is not read here and any value is accepted.
The one-hot first layer (UseInputTransform=No) and highway wrappers are not built for this layer (model_builder
refuses both).  Engine: csrc/basis_pdiag.hip (RGCN_KIND_BASIS_PDIAG).
"""
from ...common.shared_functions import glorot_variance, make_variable, make_bias
from ...model import Variable
from .message_gcn import MessageGcn


class BasisGcnWithDiag(MessageGcn):
    KIND = "basis_pdiag"

    def parse_settings(self):
        self.dropout_keep_probability = float(self.settings['DropoutKeepProbability'])
        self.n_coefficients = int(self.settings['NumberOfBasisFunctions'])

    def create_variables(self):
        if self.onehot_input:
            raise NotImplementedError("AddDiagonal=Yes with UseInputTransform=No: the one-hot first layer of "
                                      "BasisGcnWithDiag is not built")
        d_in, d_out = self.shape[0], self.shape[1]
        type_matrix_shape = (self.relation_count, self.n_coefficients)
        vertex_matrix_shape = (d_in, self.n_coefficients, d_out)
        self_matrix_shape = (d_in, d_out)
        type_diag_shape = (self.relation_count, d_out)
        var = glorot_variance([vertex_matrix_shape[0], vertex_matrix_shape[2]])
        self.W_forward = Variable("W_forward", vertex_matrix_shape, make_variable(0, var, vertex_matrix_shape))
        self.W_backward = Variable("W_backward", vertex_matrix_shape, make_variable(0, var, vertex_matrix_shape))
        self.W_self = Variable("W_self", self_matrix_shape, make_variable(0, var, self_matrix_shape))
        self.C_forward = Variable("C_forward", type_matrix_shape, make_variable(0, 1, type_matrix_shape))
        self.C_backward = Variable("C_backward", type_matrix_shape, make_variable(0, 1, type_matrix_shape))
        self.D_types_forward = Variable("D_types_forward", type_diag_shape, make_variable(0, 1, type_diag_shape))
        self.D_types_backward = Variable("D_types_backward", type_diag_shape, make_variable(0, 1, type_diag_shape))
        self.b = Variable("b", (d_out,), make_bias(d_out))

    def engine_variables(self):
        return [(self.W_forward, "W_f"), (self.W_backward, "W_b"), (self.C_forward, "C_f"), (self.C_backward, "C_b"),
                (self.D_types_backward, "D_b"), (self.D_types_forward, "D_f"), (self.W_self, "W_self"), (self.b, "b")]

    def local_get_weights(self):
        return [self.W_forward, self.W_backward, self.C_forward, self.C_backward,
                self.D_types_backward, self.D_types_forward, self.W_self, self.b]

    def local_get_regularization(self):
        return 0.0      # the reference class defines none: the chain's base 0 (model.py:111-112)
