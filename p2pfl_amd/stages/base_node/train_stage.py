"""TrainStage (reference ``stages/base_node/train_stage.py:35-184``).

Evaluate -> fit -> add the own model to the aggregator -> push partial
aggregates to train-set peers until every train-set model has been collected.
Non-members of the train set (which the reference also routed here from round
2 on, only to have their model rejected: quirk Q3) go straight to waiting for
the full aggregate.
"""

from __future__ import annotations

import time
from typing import Any, List, Optional, Type

from p2pfl_amd.commands.add_model_command import AddModelCommand
from p2pfl_amd.commands.models_agregated_command import ModelsAggregatedCommand
from p2pfl_amd.management.logger import logger
from p2pfl_amd.settings import Settings
from p2pfl_amd.stages.base_node.common import (
    DeliveryLedger,
    ReportClock,
    evaluate_and_share,
    mark_dead_train_set_members,
    model_payload,
    relay_grace,
)
from p2pfl_amd.stages.stage import Stage
from p2pfl_amd.stages.stage_factory import StageFactory


class TrainStage(Stage):
    @staticmethod
    def name() -> str:
        return "TrainStage"

    @staticmethod
    def execute(
        state: Any = None,
        communication_protocol: Any = None,
        aggregator: Any = None,
        early_stopping_fn: Any = None,
        **kwargs,
    ) -> Optional[Type[Stage]]:
        if state is None or communication_protocol is None or aggregator is None or early_stopping_fn is None:
            raise Exception("Invalid parameters on TrainStage.")
        if state.addr not in state.train_set:
            return StageFactory.get_stage("WaitAggregatedModelsStage")
        if not early_stopping_fn():
            aggregator.set_nodes_to_aggregate(state.train_set)
            mark_dead_train_set_members(state, communication_protocol, aggregator)
        if not early_stopping_fn():
            evaluate_and_share(state, communication_protocol)
        privacy = getattr(state, "privacy", None)
        start = None
        if privacy is not None:
            from p2pfl_amd.learning.step_graph import GATE  # its device work runs under the shared gate
        if not early_stopping_fn():
            if privacy is not None:
                # the weights the round starts from: the update that gets clipped is fit()'s
                # (a device copy: never beside another virtual peer's graph capture)
                with GATE.shared():
                    start = state.learner.get_parameters().clone()
            logger.info(state.addr, "Training...")
            with logger.span(state.addr, "fit", round=state.round):
                state.learner.fit()
        if not early_stopping_fn():
            learner = state.learner
            # the live weights, unordered: the aggregator's kernels read them under the
            # arena's WeightGuard (arena.reading), a one-model round reads nothing
            own = getattr(learner, "live_parameters", learner.get_parameters)()
            if privacy is not None:
                # what leaves the node is a clipped, noised copy; the learner keeps its weights
                rnd = state.round
                if rnd is None or start is None:  # stopped meanwhile: nothing is released
                    return StageFactory.get_stage("GossipModelStage")
                with logger.span(state.addr, "privatize", round=rnd), GATE.shared():
                    own = privacy.privatize(own, start, rnd)
                logger.info(state.addr, f"Privacy: {privacy.releases} updates released, epsilon = "
                            f"{privacy.epsilon():.4g} at delta = {privacy.delta:g}")
            models_added = aggregator.add_model(own, [state.addr], learner.get_num_samples()[0])
            state.changed.bump()
            communication_protocol.broadcast(
                communication_protocol.build_msg(ModelsAggregatedCommand.get_name(), models_added, round=state.round)
            )
            TrainStage._gossip_model_aggregation(state, communication_protocol, aggregator)
        return StageFactory.get_stage("GossipModelStage")

    @staticmethod
    def _gossip_model_aggregation(state: Any, protocol: Any, aggregator: Any) -> None:
        """Push partial aggregates to train-set peers until each holds every model.

        Exactly-once on a full mesh (new): a node first offers a peer ONLY its
        own model -- the one contribution nobody else can deliver -- and relays
        models of other origins to a peer only once that peer's
        ``models_aggregated`` report lists its own model (it is collecting, not
        training) and has not moved for ``GOSSIP_RELAY_GRACE``
        (on a full mesh their origins deliver them within milliseconds; on a
        sparse topology the relay follows after the grace).  A contribution on
        its way or delivered is never offered twice (:class:`DeliveryLedger`).
        With ``GOSSIP_RELAY_GRACE = 0`` every push carries everything the peer
        lacks, as in the reference (``train_stage.py:134-168``).
        """
        grace = relay_grace(state, protocol)
        ledger = DeliveryLedger(expiry=max(4 * grace, Settings.GRPC_TIMEOUT))

        def peer_has(n: str) -> List[str]:
            return state.models_aggregated.get(n, [])

        clock = ReportClock(lambda n: sorted(peer_has(n)))

        def candidates() -> List[str]:
            # A train-set peer is a candidate while it lacks some of the models
            # this node holds (per its models_aggregated reports).  The
            # reference (train_stage.py:134-139) used "its model is not in my
            # aggregate", which stops pushing as soon as the peer's model
            # arrived here even if the peer never received this node's model
            # (its own comment flags the hazard): on a partial topology that
            # leaves peers waiting for AGGREGATION_TIMEOUT.
            have = set(aggregator.get_aggregated_models())
            rnd = state.round if state.round is not None else -1
            return [
                n
                for n in protocol.get_neighbors(only_direct=False)
                if n in state.train_set and n != state.addr and (have - set(peer_has(n)))
                # a peer that announced models_ready for this round (or a later one) has
                # its aggregate: its last report of this round may never have reached this
                # node (sent while this node was still in the previous round), and pushes
                # to it would be declined until the loop's equal-rounds exit
                and state.nei_status.get(n, -1) < rnd
            ]

        def status() -> Any:
            return [(n, peer_has(n)) for n in protocol.get_neighbors(only_direct=False) if n in state.train_set]

        def model_fn(node: str) -> Any:
            token, since = clock.get(node)
            known = set(peer_has(node)) | ledger.covered(node, token)
            have = aggregator.get_aggregated_models()
            lack = set(have) - known
            if not lack or state.round is None or state.learner is None:
                return None
            model = None
            if grace > 0 and state.addr in lack:
                # own model only: every other origin delivers its own
                model, contributors, weight = aggregator.get_partial_aggregation([n for n in have if n != state.addr])
            if model is None:
                # relay only to a peer that is collecting (its report lists its
                # own model) and whose report has not moved for the grace: a peer
                # still training is not starved, its origins deliver when it is ready
                if grace > 0 and (node not in peer_has(node) or time.monotonic() - since < grace):
                    return None
                model, contributors, weight = aggregator.get_partial_aggregation(sorted(known))
            if model is None:
                return None
            msg = protocol.build_weights(
                AddModelCommand.get_name(), state.round, model_payload(state, protocol, model), contributors, weight
            )
            return ledger.attach(node, msg, token)

        protocol.gossip_weights(
            lambda: state.round is None,
            candidates,
            status,
            model_fn,
            create_connection=True,
            wakeup=state.changed,
            # a peer is reconsidered as soon as its report moves (or a period passed)
            peer_status_fn=lambda n: peer_has(n),
        )
