// resource_calls_ref.cpp — the reference's own answers on NFCPropertyModule's resource calls (FullHPMP,
// FullSP, Add / Consume / Enough of HP, MP, SP, Money, Diamond; PM:215-472), for
// tests/golden/resource_calls.json.  NFCPropertyModule.cpp is compiled where it lies, with the reference's
// kernel, AOI, event, schedule, class and element modules, around oracle/ref_server.hpp's plugin manager;
// the two interfaces the module also asks for (NFIPropertyConfigModule, NFILevelModule) are doubles of
// this harness: the base values of a level are whatever the script's last BASE / LV line handed over.
// The Player class is written here: the int properties Level, Job, OnlineCount, SceneID, GroupID, HP, MP,
// SP, MAXHP, MAXMP, MAXSP, Gold, Money, and the record CommPropertyValue of 7 rows x 3 int columns tagged
// MAXHP, MAXMP, MAXSP, so the maxima move through the module's own link (PM:127-149).
// The script of tests/resource_call_model.py (golden_script()):
//   BASE <hp> <mp> <sp>            OBJ <n>
//   <Method> <o> [v]               one of NFIPropertyModule's seventeen resource calls
//   SV <o> <group> <tag> <v>       the module's SetPropertyValue(tag, group, v)
//   LV <o> <level> <hp> <mp> <sp>  SetPropertyInt(self, "Level", level): the module's level callback rewrites
//                                  row NPG_JOBLEVEL with the base values, then FullHPMP and FullSP
//   SP <o> <name> <v>              NFCKernelModule::SetPropertyInt(name, v)
//   X                              the frame (the reference applies a call at once: nothing here)
// Objects are created through NFCKernelModule::CreateObject, so the module's own class callback adds the
// rows and sets Level 1.  Object index 99 names an NFGUID nobody has.  Every call line prints
//   A <k> <ret> : <GetPropertyInt of HP MP SP MAXHP MAXMP MAXSP Gold Money of object o>
// TEST INFRASTRUCTURE, run by tests/golden/gen_resource_calls_golden.py on a machine that has the reference.
//
// usage: resource_calls_ref <script.txt>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "NFComm/NFConfigPlugin/NFCClassModule.h"
#include "NFComm/NFConfigPlugin/NFCElementModule.h"
#include "NFComm/NFCore/NFCDataList.h"
#include "NFComm/NFKernelPlugin/NFCEventModule.h"
#include "NFComm/NFKernelPlugin/NFCKernelModule.h"
#include "NFComm/NFKernelPlugin/NFCScheduleModule.h"
#include "NFComm/NFKernelPlugin/NFCSceneAOIModule.h"
#include "NFServer/NFGameServerPlugin/NFCPropertyModule.h"
#include "ref_server.hpp"

static const char* kTags[3] = {"MAXHP", "MAXMP", "MAXSP"};
static long long g_base[3] = {0, 0, 0};  // the base value of each tag at the next level callback

class BaseValues : public NFIPropertyConfigModule {
public:
    int CalculateBaseValue(const int, const int, const std::string& tag) override {
        for (int c = 0; c < 3; c++)
            if (tag == kTags[c]) return (int)g_base[c];
        return 0;
    }
    bool LegalLevel(const int, const int) override { return true; }
};
class NoLevels : public NFILevelModule {
public:
    int AddExp(const NFGUID&, const int) override { return 0; }
};

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::ifstream in(argv[1]);
    if (!in) return 2;
    std::vector<std::vector<std::string>> lines;
    for (std::string ln; std::getline(in, ln);) {
        std::istringstream ss(ln);
        std::vector<std::string> f;
        for (std::string t; ss >> t;) f.push_back(t);
        if (!f.empty()) lines.push_back(f);
    }
    int n_obj = 0;
    size_t at = 0;
    for (; at < lines.size(); at++) {
        auto& f = lines[at];
        if (f[0] == "BASE" && f.size() == 4) {
            for (int c = 0; c < 3; c++) g_base[c] = strtoll(f[1 + c].c_str(), nullptr, 10);
        } else if (f[0] == "OBJ") {
            n_obj = atoi(f[1].c_str());
        } else {
            break;
        }
    }
    if (n_obj <= 0) return 2;

    TestPluginManager pm;
    auto prop = [](const std::string& id, const char* type) {
        return "<Property Id=\"" + id + "\" Type=\"" + type + "\" Public=\"0\" Private=\"1\" Save=\"0\" Cache=\"0\" Ref=\"0\" Upload=\"0\"/>";
    };
    pm.files["NFDataCfg/Struct/LogicClass.xml"] =
        "<XML><Class Id=\"IObject\" Type=\"TYPE_IOBJECT\" Path=\"NFDataCfg/Struct/Class/IObject.xml\" InstancePath=\"\">"
        "<Class Id=\"Player\" Type=\"TYPE_PLAYER\" Path=\"NFDataCfg/Struct/Class/Player.xml\" InstancePath=\"\"/></Class></XML>";
    pm.files["NFDataCfg/Struct/Class/IObject.xml"] =
        "<XML><Propertys>" + prop("ClassName", "string") + prop("ConfigID", "string") + "</Propertys></XML>";
    const char* names[8] = {"HP", "MP", "SP", "MAXHP", "MAXMP", "MAXSP", "Gold", "Money"};
    {
        std::string x = "<XML><Propertys>";
        for (const char* nm : {"Level", "Job", "OnlineCount", "SceneID", "GroupID"}) x += prop(nm, "int");
        for (const char* nm : names) x += prop(nm, "int");
        x += "</Propertys><Records><Record Id=\"CommPropertyValue\" Row=\"7\" Col=\"3\" Public=\"0\" Private=\"1\" Save=\"0\" "
             "Cache=\"0\" Upload=\"0\">";
        for (const char* t : kTags) x += std::string("<Col Type=\"int\" Tag=\"") + t + "\"/>";
        x += "</Record></Records></XML>";
        pm.files["NFDataCfg/Struct/Class/Player.xml"] = x;
    }
    TestLogModule log;
    NFCClassModule classes(&pm);
    NFCElementModule elements(&pm);
    NFCKernelModule kernel(&pm);
    NFCSceneAOIModule aoi(&pm);
    NFCEventModule events(&pm);
    NFCScheduleModule sched(&pm);
    BaseValues base;
    NoLevels levels;
    NFCPropertyModule props(&pm);
    pm.AddModule(typeid(NFILogModule).name(), &log);
    pm.AddModule(typeid(NFIClassModule).name(), &classes);
    pm.AddModule(typeid(NFIElementModule).name(), &elements);
    pm.AddModule(typeid(NFIKernelModule).name(), &kernel);
    pm.AddModule(typeid(NFISceneAOIModule).name(), &aoi);
    pm.AddModule(typeid(NFIEventModule).name(), &events);
    pm.AddModule(typeid(NFIScheduleModule).name(), &sched);
    pm.AddModule(typeid(NFIPropertyConfigModule).name(), &base);
    pm.AddModule(typeid(NFILevelModule).name(), &levels);
    pm.AddModule(typeid(NFIPropertyModule).name(), &props);
    std::vector<NFIModule*> all = {&log, &classes, &elements, &kernel, &aoi, &events, &sched, &base, &levels, &props};
    for (auto* m : all) m->Awake();
    for (auto* m : all) m->Init();
    for (auto* m : all) m->AfterInit();
    NFIKernelModule* km = &kernel;
    NFIPropertyModule* pmod = &props;
    km->CreateScene(1);
    if (km->RequestGroupScene(1) != 1) return 3;
    auto guid = [](int o) { return NFGUID(7, 100 + o); };
    for (int o = 0; o < n_obj; o++)
        if (!km->CreateObject(guid(o), 1, 1, "Player", "", NFCDataList())) return 3;
    int k = 0;
    for (; at < lines.size(); at++) {
        auto& f = lines[at];
        const std::string& op = f[0];
        if (op == "X") continue;
        const NFGUID g = guid(atoi(f[1].c_str()));
        const NFINT64 v = f.size() > 2 ? (NFINT64)strtoll(f[2].c_str(), nullptr, 10) : 0;
        long long ret = 0;
        if (op == "SV") {
            ret = pmod->SetPropertyValue(g, f[3], (NFIPropertyModule::NFPropertyGroup)atoi(f[2].c_str()),
                                         (int)strtoll(f[4].c_str(), nullptr, 10));
        } else if (op == "LV") {
            for (int c = 0; c < 3; c++) g_base[c] = strtoll(f[3 + c].c_str(), nullptr, 10);
            ret = km->SetPropertyInt(g, "Level", v);
        } else if (op == "SP") {
            ret = km->SetPropertyInt(g, f[2], (NFINT64)strtoll(f[3].c_str(), nullptr, 10));
        } else if (op == "FullHPMP") ret = pmod->FullHPMP(g);
        else if (op == "FullSP") ret = pmod->FullSP(g);
        else if (op == "AddHP") ret = pmod->AddHP(g, v);
        else if (op == "ConsumeHP") ret = pmod->ConsumeHP(g, v);
        else if (op == "EnoughHP") ret = pmod->EnoughHP(g, v);
        else if (op == "AddMP") ret = pmod->AddMP(g, v);
        else if (op == "ConsumeMP") ret = pmod->ConsumeMP(g, v);
        else if (op == "EnoughMP") ret = pmod->EnoughMP(g, v);
        else if (op == "AddSP") ret = pmod->AddSP(g, v);
        else if (op == "ConsumeSP") ret = pmod->ConsumeSP(g, v);
        else if (op == "EnoughSP") ret = pmod->EnoughSP(g, v);
        else if (op == "AddMoney") ret = pmod->AddMoney(g, v);
        else if (op == "ConsumeMoney") ret = pmod->ConsumeMoney(g, v);
        else if (op == "EnoughMoney") ret = pmod->EnoughMoney(g, v);
        else if (op == "AddDiamond") ret = pmod->AddDiamond(g, v);
        else if (op == "ConsumeDiamond") ret = pmod->ConsumeDiamond(g, v);
        else if (op == "EnoughDiamond") ret = pmod->EnoughDiamond(g, v);
        else {
            fprintf(stderr, "bad script line %zu\n", at);
            return 2;
        }
        printf("A %d %lld :", k++, ret);
        for (const char* nm : names) printf(" %lld", (long long)km->GetPropertyInt(g, nm));
        printf("\n");
    }
    return 0;
}
