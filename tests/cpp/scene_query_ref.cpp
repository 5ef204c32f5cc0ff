// scene_query_ref.cpp — the reference's own answers to the scene queries, for tests/golden/scene_query.json.
// A workload (noahgameframe_amd/workload.py: int / float / object properties, SwitchScene) is replayed
// window by window on the reference's NFCKernelModule (compiled from the reference tree where it lies,
// with oracle/ref_server.hpp around it; see tests/golden/gen_scene_query_golden.py), WITHOUT heartbeats:
// only properties no heartbeat program writes are queried, so the reference's values of them after a
// window's calls are its values after that frame too.  After each window's calls a fixed list of
// GetObjectByProperty / GetGroupObjectList / GetSceneOnLineList / count calls is printed, one line each:
//   Q <frame> ref <call> <a> <b> <c> <d> = <return value> : <object indices in list order>
// (the format of tests/cpp/scene_query_plugin.cpp).  TEST INFRASTRUCTURE, run by hand on a machine that
// has the reference tree.
//
// usage: scene_query_ref <workload.nfio>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include <sys/syscall.h>
#include <time.h>
#include <unistd.h>

#include "NFComm/NFKernelPlugin/NFCEventModule.h"
#include "NFComm/NFKernelPlugin/NFCKernelModule.h"
#include "NFComm/NFKernelPlugin/NFCScheduleModule.h"
#include "NFComm/NFKernelPlugin/NFCSceneAOIModule.h"
#include "NFComm/NFConfigPlugin/NFCClassModule.h"
#include "NFComm/NFConfigPlugin/NFCElementModule.h"
#include "../../oracle/nfio.h"
#include "../../oracle/ref_server.hpp"

extern "C" int clock_gettime(clockid_t clk, struct timespec* ts) {  // NFGetTime(): the session clock
    if (clk == CLOCK_REALTIME) {
        ts->tv_sec = g_now / 1000;
        ts->tv_nsec = (g_now % 1000) * 1000000;
        return 0;
    }
    return (int)syscall(SYS_clock_gettime, clk, ts);
}

// NFCSceneAOIModule's own common callbacks are dropped, as oracle/ref_session.cpp does: its OnGroupEvent
// releases the whole group a player leaves (AOI:389-393: ReleaseGroupScene destroys the group's other
// members), a side effect of that module's default configuration and not of the kernel module's queries.
struct QueryKernel : NFCKernelModule {
    using NFCKernelModule::NFCKernelModule;
    void DropCommonCallbacks() {
        mtCommonClassCallBackList.clear();
        mtCommonPropertyCallBackList.clear();
        mtCommonRecordCallBackList.clear();
    }
};

static std::string cstr(const uint8_t* p) { return std::string((const char*)p, strnlen((const char*)p, 32)); }

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    nfio_file wf;
    if (nfio_read(argv[1], &wf)) return 2;
    auto A = [&](const char* n) {
        nfio_arr* a = nfio_get(&wf, n);
        if (!a) { fprintf(stderr, "missing %s\n", n); exit(2); }
        return a;
    };
    int64_t* cfg = (int64_t*)A("cfg")->data;
    const int64_t N = cfg[0], NI = cfg[1], NF = cfg[2], NC = cfg[3], NT = cfg[7];
    const int64_t NO = ((int64_t*)A("n_oprops")->data)[0], NP = NI + NF + NO;
    uint8_t* pnames = (uint8_t*)A("prop_names")->data;
    std::vector<std::string> pname(NP), cname = {"NPC", "Player"};
    for (int p = 0; p < NP; p++) pname[p] = cstr(pnames + 32 * p);

    TestPluginManager pm;
    write_class_schema(pm, wf, pname, cname, NI, NF, NC, 0);
    TestLogModule log;
    NFCClassModule classes(&pm);
    NFCElementModule elements(&pm);
    QueryKernel kernel(&pm);
    NFCScheduleModule sched(&pm);
    NFCSceneAOIModule aoi(&pm);
    NFCEventModule events(&pm);
    pm.AddModule(typeid(NFILogModule).name(), &log);
    pm.AddModule(typeid(NFIClassModule).name(), &classes);
    pm.AddModule(typeid(NFIElementModule).name(), &elements);
    pm.AddModule(typeid(NFIKernelModule).name(), &kernel);
    pm.AddModule(typeid(NFISceneAOIModule).name(), &aoi);
    pm.AddModule(typeid(NFIEventModule).name(), &events);
    pm.AddModule(typeid(NFIScheduleModule).name(), &sched);
    std::vector<NFIModule*> all = {&log, &classes, &elements, &kernel, &aoi, &events, &sched};
    for (auto* m : all) m->Awake();
    for (auto* m : all) {
        m->Init();
        if (m == &aoi) kernel.DropCommonCallbacks();
    }
    NFIKernelModule* km = &kernel;

    int64_t* gh = (int64_t*)A("guid_head")->data;
    int64_t* gd = (int64_t*)A("guid_data")->data;
    int32_t* sc = (int32_t*)A("scene")->data;
    int32_t* gr = (int32_t*)A("group")->data;
    uint8_t* cl = (uint8_t*)A("cls")->data;
    int64_t* ii = (int64_t*)A("init_i")->data;
    double* ff = (double*)A("init_f")->data;
    int64_t* ioh = (int64_t*)A("init_oh")->data;
    int64_t* iod = (int64_t*)A("init_od")->data;
    nfio_arr* swa = A("sw_tick");
    const int64_t NW = (int64_t)swa->shape[0];
    int32_t* sw_tick = (int32_t*)swa->data;
    int32_t* sw_obj = (int32_t*)A("sw_obj")->data;
    int32_t* sw_scene = (int32_t*)A("sw_scene")->data;
    int32_t* sw_group = (int32_t*)A("sw_group")->data;
    float* sw_x = (float*)A("sw_x")->data;
    float* sw_y = (float*)A("sw_y")->data;
    float* sw_z = (float*)A("sw_z")->data;
    std::map<NFGUID, int> index;
    for (int64_t o = 0; o < N; o++) index[NFGUID(gh[o], gd[o])] = (int)o;
    // scenes and their groups 1..G (CreateScene / RequestGroupScene); a group beyond them is requested
    // in the window of the first SwitchScene into it
    std::map<int, int> groups;
    for (int64_t o = 0; o < N; o++) groups[sc[o]] = std::max(groups[sc[o]], gr[o]);
    for (auto& kv : groups) {
        km->CreateScene(kv.first);
        for (int g = 1; g <= kv.second; g++)
            if (km->RequestGroupScene(kv.first) != g) return 3;
    }
    for (int64_t o = 0; o < N; o++) {
        NFCDataList arg;
        for (int p = 0; p < NP; p++) {
            if (pname[p] == "SceneID" || pname[p] == "GroupID") continue;
            arg.Add(pname[p]);
            if (p < NI) arg.Add((NFINT64)ii[p * N + o]);
            else if (p < NI + NF) arg.Add(ff[(p - NI) * N + o]);
            else arg.Add(NFGUID(ioh[(p - NI - NF) * N + o], iod[(p - NI - NF) * N + o]));
        }
        if (!km->CreateObject(NFGUID(gh[o], gd[o]), sc[o], gr[o], cname[cl[o]], "", arg)) return 3;
    }
    for (auto* m : all) m->AfterInit();
    for (auto* m : all) m->ReadyExecute();

    nfio_arr* xa = A("x_tick");
    const int64_t NX = (int64_t)xa->shape[0];
    int32_t* x_tick = (int32_t*)xa->data;
    int32_t* x_obj = (int32_t*)A("x_obj")->data;
    int32_t* x_pid = (int32_t*)A("x_pid")->data;
    uint64_t* x_bits = (uint64_t*)A("x_bits")->data;
    uint64_t* x_bits_h = (uint64_t*)A("x_bits_h")->data;
    std::vector<int32_t> cur_sc(sc, sc + N), cur_gr(gr, gr + N);
    int pid_level = -1, pid_gold = -1, pid_x = -1;
    for (int p = 0; p < NP; p++) {
        if (pname[p] == "Level") pid_level = p;
        if (pname[p] == "Gold") pid_gold = p;
        if (pname[p] == "X") pid_x = p;
    }
    const int pid_master = (int)(NI + NF) + 1;  // MasterID
    if (pid_level < 0 || pid_gold < 0 || pid_x < 0 || pid_master >= NP) return 4;

    auto line = [&](int t, const char* call, long long a, long long b, long long c, long long d, long long ret,
                    const NFIDataList& l) {
        printf("Q %d ref %s %lld %lld %lld %lld = %lld :", t, call, a, b, c, d, ret);
        for (int i = 0; i < l.GetCount(); i++) printf(" %d", index.at(l.Object(i)));
        printf("\n");
    };
    auto ask = [&](int t, int64_t gold_value) {
        auto gobp_i = [&](int scene, int pid, int64_t v) {
            NFCDataList arg, l;
            arg.Add((NFINT64)v);
            const int r = km->GetObjectByProperty(scene, pname[pid], arg, l);
            line(t, "gobp_i", scene, pid, v, 0, r, l);
        };
        auto gobp_o = [&](int scene, int pid, const NFGUID& v) {
            NFCDataList arg, l;
            arg.Add(v);
            const int r = km->GetObjectByProperty(scene, pname[pid], arg, l);
            line(t, "gobp_o", scene, pid, v.nHead64, v.nData64, r, l);
        };
        for (int s : {1, 2, 3}) gobp_i(s, pid_level, 17);
        gobp_i(1, pid_level, 42);
        gobp_i(1, pid_level, 17 + (1ll << 32));  // an argument >= 2^32 (a property of 2^32 + 17 reads 17)
        gobp_i(2, pid_gold, gold_value);         // the value of the window's last SetPropertyInt(Gold)
        gobp_i(1, pid_x, 0);                     // an int argument on a float property
        gobp_i(1, pid_x, 3);
        gobp_i(1, pid_master, 0);                // ... on an object property
        gobp_i(9, pid_level, 17);                // no such scene
        {   // an object argument: the MasterID the first player of scene 1 holds now
            NFCDataList pl;
            km->GetSceneOnLineList(1, pl);
            const NFGUID v = km->GetPropertyObject(pl.Object(0), pname[pid_master]);
            gobp_o(1, pid_master, v);
            gobp_o(2, pid_master, v);
            gobp_o(1, pid_master, NFGUID(v.nHead64 + 1, v.nData64));
            gobp_o(1, pid_level, NFGUID());      // an object argument on an int property
            gobp_o(1, pid_level, v);
            NFCDataList arg, l;
            arg.Add(0.0);
            line(t, "gobp_f", 1, pid_x, 0, 0, km->GetObjectByProperty(1, pname[pid_x], arg, l), l);
        }
        for (auto sg : {std::make_pair(1, 2), std::make_pair(3, 6), std::make_pair(1, 99)}) {
            const int s = sg.first, g = sg.second;
            NFCDataList l0, l1, l2, l3, l4, pl;
            bool r = km->GetGroupObjectList(s, g, l0);
            line(t, "ggol", s, g, -1, 0, r, l0);
            r = km->GetGroupObjectList(s, g, l1, true);
            line(t, "ggol", s, g, 1, 0, r, l1);
            r = km->GetGroupObjectList(s, g, l2, false);
            line(t, "ggol", s, g, 0, 0, r, l2);
            r = km->GetGroupObjectList(s, g, "NPC", l3);
            line(t, "ggol_c", s, g, 0, -1, r, l3);
            km->GetGroupObjectList(s, g, pl, true);
            const NFGUID self = pl.GetCount() ? pl.Object(pl.GetCount() / 2) : NFGUID();
            r = km->GetGroupObjectList(s, g, "Player", self, l4);
            line(t, "ggol_c", s, g, 1, pl.GetCount() ? index.at(self) : -1, r, l4);
        }
        NFCDataList l, none;
        line(t, "sol", 2, 0, 0, 0, km->GetSceneOnLineList(2, l), l);
        line(t, "soc", 1, -1, 0, 0, km->GetSceneOnLineCount(1), none);
        line(t, "soc", 3, 6, 0, 0, km->GetSceneOnLineCount(3, 6), none);
        line(t, "soc", 2, 3, 0, 0, km->GetSceneOnLineCount(2, 3), none);
        line(t, "soc", 9, -1, 0, 0, km->GetSceneOnLineCount(9), none);
        line(t, "olc", 0, 0, 0, 0, km->GetOnLineCount(), none);
    };

    int64_t xi = 0, wi = 0, gold_value = 1;
    for (int t = 0; t < NT; t++) {
        for (; wi < NW && sw_tick[wi] == t; wi++) {
            const int o = sw_obj[wi];
            if (sw_scene[wi] >= 0) { cur_sc[o] = sw_scene[wi]; cur_gr[o] = sw_group[wi]; }
            while (groups[cur_sc[o]] < cur_gr[o])
                if (km->RequestGroupScene(cur_sc[o]) != ++groups[cur_sc[o]]) return 3;
            if (!km->SwitchScene(NFGUID(gh[o], gd[o]), cur_sc[o], cur_gr[o], sw_x[wi], sw_y[wi], sw_z[wi], 0.0f, NFCDataList())) {
                fprintf(stderr, "SwitchScene of object %d to (%d, %d) in window %d refused (SceneID %lld, GroupID %lld)\n", o, cur_sc[o], cur_gr[o], t,
                        (long long)km->GetPropertyInt(NFGUID(gh[o], gd[o]), "SceneID"), (long long)km->GetPropertyInt(NFGUID(gh[o], gd[o]), "GroupID"));
                return 5;
            }
        }
        for (; xi < NX && x_tick[xi] == t; xi++) {
            const NFGUID g(gh[x_obj[xi]], gd[x_obj[xi]]);
            const int p = x_pid[xi];
            if (p == pid_level || p == pid_gold) {  // (the properties queried; the others are the programs')
                km->SetPropertyInt(g, pname[p], (NFINT64)x_bits[xi]);
                if (p == pid_gold) gold_value = (int64_t)x_bits[xi];
            } else if (p >= NI + NF) {
                km->SetPropertyObject(g, pname[p], NFGUID((int64_t)x_bits_h[xi], (int64_t)x_bits[xi]));
            }
        }
        ask(t, gold_value);
    }
    return 0;
}
