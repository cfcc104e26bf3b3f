"""Plugin registry (reference: code/common/model_builder.py): maps `Encoder.Name` and its flags to a
chain of components.  Only the hot-path family is built: `Name=gcn_basis` with UseOutputTransform=No or -- for the
Concatenation=No stacks (BasisGcn, BasisGcnTimesDiag, BasisGcnWithDiag) -- Yes (the dense AffineTransform
[InternalEncoderDimension, CodeDimension] over the top layer, :131-135,170-177), SkipConnections
None or Highway (every layer wrapped in extras/highway_layer.py; UseInputTransform=Yes only) and none of the
experimental layer flags except DiagonalCoefficients=Yes (BasisGcnTimesDiag, with the reference's precedence over
Concatenation; UseInputTransform=Yes and SkipConnections=None only) and AddDiagonal=Yes (BasisGcnWithDiag; the same two
conditions, and with Concatenation=No and DiagonalCoefficients=No only: the reference lets AddDiagonal override both
silently, a contradictory file is refused here) -- UseInputTransform=Yes (exactly
settings/gcn_block.exp and settings/gcn_basis.exp) or, for the basis kind, UseInputTransform=No: the featureless encoder
whose first layer reads one-hot entity ids (:140-165,277-283); everything else raises NotImplementedError naming SURVEY.md section 2's
out-of-scope row instead of silently building something different.  `Name=embedding` (settings/distmult.exp; :27-41) builds
the graph-less DistMult baseline, RelationEmbedding over the bias-free lookup AffineTransform; a file that says
`Name=embedding` and also carries keys of a graph-convolution stack (NumberOfLayers, Concatenation, ...) is refused as
contradictory rather than having its layers dropped silently."""
from ..decoders.bilinear_diag import BilinearDiag
from ..encoders.affine_transform import AffineTransform
from ..encoders.message_gcns.gcn_basis import BasisGcn
from ..encoders.message_gcns.gcn_basis_concat import ConcatGcn
from ..encoders.message_gcns.gcn_basis_plus_diag import BasisGcnWithDiag
from ..encoders.message_gcns.gcn_basis_times_diag import BasisGcnTimesDiag
from ..encoders.relation_embedding import RelationEmbedding
from ..extras.graph_representations import Representation
from ..extras.highway_layer import HighwayLayer


def _flag(settings, key, default="No"):
    return settings[key] if key in settings else default


# Keys of the [Encoder] section that configure a stack of graph-convolution layers.  The reference's `embedding` branch reads
# none of them (model_builder.py:27-41): a file that names the graph-less encoder AND describes a layer stack would get its
# layers dropped silently, so -- as with AddDiagonal beside Concatenation below -- the contradictory file is refused.
_LAYER_STACK_KEYS = ('NumberOfLayers', 'NumberOfBasisFunctions', 'InternalEncoderDimension', 'DropoutKeepProbability',
                     'UseInputTransform', 'UseOutputTransform', 'Concatenation', 'AddDiagonal', 'DiagonalCoefficients',
                     'SkipConnections', 'StoreEdgeData', 'RandomInput', 'PartiallyRandomInput')


def build_encoder(encoder_settings, triples):
    name = encoder_settings['Name']
    if name == "embedding":
        stack_keys = [key for key in _LAYER_STACK_KEYS if key in encoder_settings]
        if stack_keys:
            raise NotImplementedError("Name=embedding beside %s: the embedding encoder has no graph-convolution layers and the "
                                      "reference would ignore these keys silently (model_builder.py:27-41); the contradictory "
                                      "file is refused -- settings/distmult.exp carries none of them" % ", ".join(stack_keys))
        # model_builder.py:27-41; the model is built from EntityCount and CodeDimension only, as the reference's is
        input_shape = [int(encoder_settings['EntityCount']), int(encoder_settings['CodeDimension'])]
        embedding = AffineTransform(input_shape, encoder_settings, onehot_input=True, use_bias=False,
                                    use_nonlinearity=False)
        return RelationEmbedding(input_shape, encoder_settings, next_component=embedding)
    if name != "gcn_basis":
        raise NotImplementedError("encoder '%s' is outside the accelerated path (SURVEY.md section 2); only 'gcn_basis' "
                                  "(ConcatGcn / BasisGcn stacks) and 'embedding' (the DistMult baseline) are built" % name)
    input_transform = _flag(encoder_settings, 'UseInputTransform', None)
    if input_transform not in ("Yes", "No"):
        raise NotImplementedError("UseInputTransform must be Yes or No (the reference reads it unconditionally, "
                                  "model_builder.py:140), got %r" % (input_transform,))
    # the reference picks the layer class in this order (model_builder.py:285-294): AddDiagonal, DiagonalCoefficients,
    # StoreEdgeData, Concatenation -- AddDiagonal (BasisGcnWithDiag) would silently override DiagonalCoefficients and
    # Concatenation: a file that sets it beside either contradicts itself and is refused (honouring the reference's precedence
    # is a follow-up); Concatenation, behind DiagonalCoefficients, loses to it; StoreEdgeData=Yes stays refused
    # whatever the layer (the training loop reads it too, train.py:242)
    add_diag = _flag(encoder_settings, 'AddDiagonal') == "Yes"
    if add_diag:
        for key in ('Concatenation', 'DiagonalCoefficients'):
            if _flag(encoder_settings, key) == "Yes":
                raise NotImplementedError("AddDiagonal=Yes with %s=Yes: the reference lets AddDiagonal win silently "
                                          "(model_builder.py:285-292); the contradictory file is refused" % key)
    times_diag = _flag(encoder_settings, 'DiagonalCoefficients') == "Yes"
    concat = _flag(encoder_settings, 'Concatenation') == "Yes" and not times_diag
    if input_transform == "No" and concat:
        raise NotImplementedError("UseInputTransform=No with Concatenation=Yes: the reference's one-hot branch of "
                                  "ConcatGcn cannot execute (gcn_basis_concat.py:18-19,42-46)")
    for key in ('StoreEdgeData', 'RandomInput', 'PartiallyRandomInput'):
        if _flag(encoder_settings, key) == "Yes":
            raise NotImplementedError("%s=Yes selects a reference variant outside the hot path" % key)
    output_transform = _flag(encoder_settings, 'UseOutputTransform') == "Yes"
    if output_transform and concat:
        # (the engine runs the layer over the block kind too; the plugin holds it back: the block kind is the one with
        # sharding, capture and the deferred-join schedule, none of which is built for the layer -- INTEGRATION.md)
        raise NotImplementedError("UseOutputTransform=Yes selects a reference variant outside the hot path beside "
                                  "Concatenation=Yes (the plugin builds the output transform over Concatenation=No stacks)")
    skip = _flag(encoder_settings, 'SkipConnections', 'None')
    if skip not in ('None', 'Highway'):
        raise NotImplementedError("SkipConnections other than None")
    if skip == 'Highway' and input_transform == "No":
        raise NotImplementedError("SkipConnections=Highway with UseInputTransform=No is the one-hot follow-up: the "
                                  "reference gives the one-hot first layer no highway layer while the layers above it "
                                  "get one (model_builder.py:304-305), which the engine does not build")

    if times_diag and input_transform == "No":
        raise NotImplementedError("DiagonalCoefficients=Yes with UseInputTransform=No: the one-hot first layer of "
                                  "BasisGcnTimesDiag is not built")
    if times_diag and skip == 'Highway':
        raise NotImplementedError("DiagonalCoefficients=Yes with SkipConnections=Highway: highway layers around "
                                  "BasisGcnTimesDiag are not built")

    if add_diag and input_transform == "No":
        raise NotImplementedError("AddDiagonal=Yes with UseInputTransform=No: the one-hot first layer of "
                                  "BasisGcnWithDiag is not built")
    if add_diag and skip == 'Highway':
        raise NotImplementedError("AddDiagonal=Yes with SkipConnections=Highway: highway layers around "
                                  "BasisGcnWithDiag are not built")

    graph = Representation(triples, encoder_settings)
    input_shape = [int(encoder_settings['EntityCount']), int(encoder_settings['InternalEncoderDimension'])]
    internal_shape = [int(encoder_settings['InternalEncoderDimension']),
                      int(encoder_settings['InternalEncoderDimension'])]
    projection_shape = [int(encoder_settings['InternalEncoderDimension']), int(encoder_settings['CodeDimension'])]
    relation_shape = [int(encoder_settings['EntityCount']), int(encoder_settings['CodeDimension'])]
    if not output_transform and int(encoder_settings['CodeDimension']) != internal_shape[1]:
        raise NotImplementedError("CodeDimension != InternalEncoderDimension needs UseOutputTransform=Yes")
    layers = int(encoder_settings['NumberOfLayers'])

    if input_transform == "Yes":
        encoding = AffineTransform(input_shape, encoder_settings, next_component=graph, onehot_input=True,
                                   use_bias=True, use_nonlinearity=True)
    else:
        encoding = graph      # RandomInput / PartiallyRandomInput are refused above: the layers sit on the graph itself
    encoding = apply_basis_gcn(encoder_settings, encoding, internal_shape, layers,
                               onehot_first=input_transform == "No")
    if output_transform:      # (model_builder.py:170-177: applied whenever the flag says Yes, also at equal dimensions)
        encoding = AffineTransform(projection_shape, encoder_settings, next_component=encoding, onehot_input=False,
                                   use_nonlinearity=False, use_bias=True)
    return RelationEmbedding(relation_shape, encoder_settings, next_component=encoding)


def apply_basis_gcn(encoder_settings, encoding, internal_shape, layers, onehot_first=False):
    concat = 'Concatenation' in encoder_settings and encoder_settings['Concatenation'] == "Yes"
    if _flag(encoder_settings, 'AddDiagonal') == "Yes":                # the first flag checked (model_builder.py:285-286)
        layer_class = BasisGcnWithDiag
    elif _flag(encoder_settings, 'DiagonalCoefficients') == "Yes":     # ahead of Concatenation (model_builder.py:287-292)
        layer_class = BasisGcnTimesDiag
    else:
        layer_class = ConcatGcn if concat else BasisGcn
    highway = _flag(encoder_settings, 'SkipConnections', 'None') == 'Highway'
    for layer in range(layers):
        onehot_input = onehot_first and layer == 0
        new_encoding = layer_class(internal_shape, encoder_settings, next_component=encoding,
                                   onehot_input=onehot_input, use_nonlinearity=layer < layers - 1)
        if highway and not onehot_input:       # (model_builder.py:304-305)
            encoding = HighwayLayer(internal_shape, next_component=new_encoding, next_component_2=encoding)
        else:
            encoding = new_encoding
    return encoding


def build_decoder(encoder, decoder_settings):
    if decoder_settings['Name'] == "bilinear-diag":
        return BilinearDiag(encoder, decoder_settings)
    raise NotImplementedError("decoder '%s' is not in any BASELINE config (SURVEY.md section 2)"
                              % decoder_settings['Name'])
