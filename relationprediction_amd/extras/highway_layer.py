"""Highway skip connection around one graph-convolution layer (reference: code/extras/highway_layer.py, placed by
apply_basis_gcn under SkipConnections=Highway, code/common/model_builder.py:304-305).

    gates = sigmoid(code_2 . W + b)                 code_2 = what lies under the wrapped layer (next_component_2)
    out   = gates * code_1 + (1 - gates) * code_2   code_1 = the wrapped layer's result       (next_component)

`W ~ N(0, glorot_variance(shape))`, `b = ones` (:25-29); `get_weights()` appends `[W, b]` behind the wrapped layer's
weights.  The arithmetic runs inside the engine (csrc/highway.hip, RGCN_SKIP_HIGHWAY): the activation the engine
reports for the wrapped layer's index IS the highway layer's output, so this component contributes its two weights
and reads that activation.  As in the reference the constructor takes no settings and does not call Model.__init__.
"""
from ..common.shared_functions import glorot_variance, make_variable, make_bias
from ..model import Model, Variable
from ..runtime import EncoderRuntime


class HighwayLayer(Model):
    W = None
    b = None

    def __init__(self, shape, next_component=None, next_component_2=None):
        self.next_component = next_component
        self.next_component_2 = next_component_2
        self.shape = shape
        if next_component is not None:
            next_component.highway_layer = self      # the runtime finds the wrapper of a layer here

    def local_initialize_train(self):
        variance = glorot_variance(self.shape)
        self.W = Variable("W_highway", tuple(self.shape), make_variable(0, variance, tuple(self.shape)))
        self.b = Variable("b_highway", (self.shape[1],), make_bias(self.shape[1], init=1))

    def local_get_weights(self):
        return [self.W, self.b]

    def engine_variables(self):
        return [(self.W, "W_highway"), (self.b, "b_highway")]

    def compute_vertex_embeddings(self, mode='train'):
        return self.next_component.compute_vertex_embeddings(mode=mode)      # the engine's post-highway H_l

    def get_all_codes(self, mode='train'):
        collected_messages = self.compute_vertex_embeddings(mode=mode)
        return collected_messages, None, collected_messages

    def get_all_subject_codes(self, mode='train'):
        return self.compute_vertex_embeddings(mode=mode)

    def get_all_object_codes(self, mode='train'):
        return self.compute_vertex_embeddings(mode=mode)

    def backward(self, upstream):
        """Top of the stack: `upstream` is dL/dcodes and starts the engine's backward pass; further down the runtime is
        handed through.  Gradients in get_weights() order: everything below, the wrapped layer's, then W and b."""
        layer = self.next_component
        rt = upstream if isinstance(upstream, EncoderRuntime) else layer.get_runtime().backward(upstream)
        return layer.backward(rt) + [rt.grad("%s%d" % (base, layer.layer_index)) for _, base in self.engine_variables()]
