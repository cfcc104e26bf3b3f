"""Input embedding layer (reference: code/encoders/affine_transform.py).

With `onehot_input=True` the layer is a lookup table plus bias plus relu: `H0 = relu(W + b)`
(:63-83), `W ~ N(0, glorot_variance(shape))`, `b = 0` (:24-28).  That is the configuration the
gcn_basis settings build (UseInputTransform=Yes, model_builder.py:141-146), wired to the engine's
kernel k_input_fwd.  The second one built is the bias-free lookup of `Name=embedding`
(model_builder.py:27-41: onehot_input=True, use_bias=False, use_nonlinearity=False, nothing beneath
it): the codes ARE `W`, `b` is created and checkpointed but never read, and the component owns a
graph-less runtime (runtime.EmbeddingRuntime, an RGCN_KIND_EMBEDDING engine context).  The third is
the dense branch of UseOutputTransform=Yes (model_builder.py:170-177: onehot_input=False,
use_bias=True, use_nonlinearity=False, over the graph-convolution stack): `codes = H_L . W + b`, run
by the stack's engine context (rgcn_config_ext::code_dim, csrc/output_transform.hip); the component
contributes `W_out [d, c]` and `b_out [c]` and returns the engine's codes.
"""
from ..common.shared_functions import glorot_variance, make_variable, make_bias
from ..extras.graph_representations import Representation
from ..model import Model, Variable
from ..runtime import EmbeddingRuntime, EncoderRuntime


class AffineTransform(Model):
    W = None
    b = None
    use_nonlinearity = False
    onehot_input = False
    use_bias = True
    shape = None

    def __init__(self, shape, settings, next_component=None, use_nonlinearity=False, onehot_input=False,
                 use_bias=True):
        Model.__init__(self, next_component, settings)
        self.shape = shape
        self.use_nonlinearity = use_nonlinearity
        self.use_bias = use_bias
        self.onehot_input = onehot_input
        # the lookup of Name=embedding: bias-free, linear, with no component beneath it
        self.lookup = bool(onehot_input and not use_bias and not use_nonlinearity and next_component is None)
        self._lookup_runtime = None         # (the graph's runtime lives on the Representation; only the lookup owns one)
        # the output transform of UseOutputTransform=Yes: dense, biased, linear, over a component chain
        self.dense = bool(not onehot_input and use_bias and not use_nonlinearity and next_component is not None)
        if not (onehot_input and use_bias and use_nonlinearity) and not self.lookup and not self.dense:
            raise NotImplementedError(
                "AffineTransform is implemented as the encoder's input layer (onehot_input=True, use_bias=True, "
                "use_nonlinearity=True), as the 'embedding' encoder's lookup (onehot_input=True, use_bias=False, "
                "use_nonlinearity=False, no component beneath it) and as the output transform of "
                "UseOutputTransform=Yes (onehot_input=False, use_bias=True, use_nonlinearity=False, over a layer stack)")

    def _representation(self):
        comp = self.next_component
        while comp is not None and not isinstance(comp, Representation):
            comp = comp.next_component
        if comp is None:
            raise NotImplementedError("the output transform sits over a graph-convolution stack")
        return comp

    def local_initialize_train(self):
        variance = glorot_variance(self.shape)
        w_name, b_name = ("W_out", "b_out") if self.dense else ("W_emb", "b_emb")
        self.W = Variable(w_name, self.shape, make_variable(0, variance, tuple(self.shape)))
        self.b = Variable(b_name, (self.shape[1],), make_bias(self.shape[1]))
        if self.dense:      # the stack's runtime, built when the first layer is asked, finds the layer here
            self._representation()._output_transform = self

    def local_get_weights(self):
        return [self.W, self.b]

    def needs_graph(self):
        return False if self.lookup else Model.needs_graph(self)

    def get_runtime(self):
        return self._runtime() if self.lookup else Model.get_runtime(self)

    def _runtime(self):
        if self.lookup:
            if self._lookup_runtime is None:
                if self.W is None:
                    raise RuntimeError("initialize_train() has not drawn the weights yet")
                self._lookup_runtime = EmbeddingRuntime(self)
            return self._lookup_runtime
        rep = self.next_component
        if rep.runtime is None:
            raise RuntimeError("the encoder has no graph-convolution layer above the input layer")
        return rep.runtime

    def get_all_codes(self, mode='train'):
        if self.dense:
            h = self.next_component.get_runtime().forward(mode).codes()
        else:
            h = self._runtime().forward(mode).activation(0)
        return h, None, h

    def get_all_subject_codes(self, mode='train'):
        return self.get_all_codes(mode)[0]

    def get_all_object_codes(self, mode='train'):
        return self.get_all_codes(mode)[2]

    def backward(self, runtime):
        if self.dense:       # `runtime` is dL/dcodes [V,c]: it starts the engine's backward pass, the stack reports below
            rt = runtime if isinstance(runtime, EncoderRuntime) else self.next_component.get_runtime().backward(runtime)
            return self.next_component.backward(rt) + [rt.grad("W_out"), rt.grad("b_out")]
        if self.lookup:      # `runtime` is dL/dcodes [V,d], handed down by RelationEmbedding: it IS W's gradient
            rt = self._runtime().backward(runtime)
            return [rt.grad("W_emb"), rt.grad("b_emb")]
        return self.next_component.backward(runtime) + [runtime.grad("W_emb"), runtime.grad("b_emb")]
